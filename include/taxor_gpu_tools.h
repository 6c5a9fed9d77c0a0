/*
 * taxor_gpu_tools.h -- everything libtaxor_gpu.so exports BESIDE the drop-in seam (taxor_gpu.h): the batch call split into its
 * phases for callers that keep a batch resident, run statistics and measurement aids, the stage entry points
 * the parity tests check one by one against the oracle, index construction on the device (8(f) #3), diagnosis of indexes this
 * library did not write (record schema probe, arithmetic / layout variant scan; 8(f) #2), the synthetic workload generator and
 * the device side of the .gz reader.  Same conventions as taxor_gpu.h; a binding of the reference needs none of this.
 */
#ifndef TAXOR_GPU_TOOLS_H
#define TAXOR_GPU_TOOLS_H

#include "taxor_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- more about a resident index */
/* current hash seed of one IXF (construction on the device may have redrawn it) */
uint64_t taxor_gpu_index_ixf_seed(const taxor_gpu_index *idx, uint64_t ixf);
/* number of leaf runs (= tuples a threshold-0 read produces) and IXF tree depth */
uint64_t taxor_gpu_index_leaf_runs(const taxor_gpu_index *idx);
uint32_t taxor_gpu_index_depth(const taxor_gpu_index *idx);
/* Measurement aid (SURVEY.md 8(d) "measured gather ceiling"): read about want_bytes of IXF `ixf` as whole rows at
 * random row indices with the access shape of the query kernel's dense phase (16 B per lane, neighbouring lanes on
 * one row) and nothing else, `reps` times; reports the requested-bytes rate and the bytes read per row. */
int taxor_gpu_gather_ceiling(taxor_gpu_index *idx, uint64_t ixf, uint64_t want_bytes, int reps, double *gb_per_s,
                             uint64_t *row_bytes);
/* the same over up to n_ixf consecutive, equally shaped IXFs starting at `ixf` (e.g. all children of a synthetic index:
 * one 128-bin IXF of 68 MB sits in the caches, a thousand of them do not); *span_used = how many were covered */
int taxor_gpu_gather_ceiling_span(taxor_gpu_index *idx, uint64_t ixf, uint64_t n_ixf, uint64_t want_bytes, int reps,
                                  double *gb_per_s, uint64_t *row_bytes, uint64_t *span_used);
/* Calibration aid for the traffic counter (rocprofv3 --pmc FETCH_SIZE is calibrated for wide coalesced reads only):
 * launches with a KNOWN request count in the two access shapes of the query kernel, nothing else.  pattern 0 = whole rows
 * at random row indices (dense phase), pattern 1 = one 16-B load per lane, every lane on a row of its own (sparse phase);
 * nt = non-temporal loads.  One warm-up launch plus `reps` timed ones, all of the same size; reports the requested-bytes
 * rate and, per launch, the requested bytes (pattern 0: rows x row bytes; pattern 1: loads x 16) and the request count
 * (rows / loads). */
int taxor_gpu_gather_pattern(taxor_gpu_index *idx, uint64_t ixf, int pattern, int nt, uint64_t want_bytes, int reps,
                             double *gb_per_s, uint64_t *bytes_per_launch, uint64_t *requests_per_launch);
/* Index construction helpers for synthetic / planted indexes (what a GPU builder would use):
 * fill one IXF with seeded pseudo-random fingerprints (behaves like non-matching bins, FPR 2^-8),
 * overwrite one bin column (rows = 3*seg_len bytes), read an IXF back (to hand the same bytes to a
 * checker). */
int taxor_gpu_index_fill_random(taxor_gpu_index *idx, uint64_t ixf, uint64_t seed);
int taxor_gpu_index_upload_bin(taxor_gpu_index *idx, uint64_t ixf, uint64_t bin, const uint8_t *column,
                               uint64_t rows);
int taxor_gpu_index_download_ixf(const taxor_gpu_index *idx, uint64_t ixf, uint8_t *data, uint64_t len);
/* GPU construction of the fingerprint columns of one IXF, in place (the reference builds on
 * the CPU: src/hixf/build/construct_ixf.cpp:50-165, add_bin_elements + reseed loop).  keys = the bins' key lists
 * concatenated (distinct within a bin), key_off[bins+1]; bins without keys keep their content.  All bins are peeled
 * at once in synchronous rounds (taxor_amd/csrc/builder.hip); if a bin does not peel the IXF is re-seeded and rebuilt,
 * like the reference.  On success the IXF carries *seed_out (also written into the resident index); *rounds_out =
 * peeling rounds of the slowest chunk.  The columns are a function of (keys, seed) alone: two builds are byte-identical.
 * Every key is looked up in the finished columns before the call returns.  The index must not be searched meanwhile.  The
 * builder's scratch (peeling state of one chunk, <= 3 GB unless one bin needs more; the union table; mark bytes) stays with the
 * index for its next build and is released by taxor_gpu_index_destroy. */
int taxor_gpu_index_build_ixf(taxor_gpu_index *idx, uint64_t ixf, const uint64_t *keys, const uint64_t *key_off,
                              uint64_t seed0, uint64_t *seed_out, uint32_t *rounds_out);
/* The whole hierarchy at once (the back end of hierarchical_build.cpp:27-236): key_off[total_bins + 1] indexes `keys`
 * per technical bin in the index's bin order (all bins of IXF 0, then IXF 1, ...); LEAF bins bring their keys
 * (distinct within a bin; a split user bin brings one part per technical bin), MERGED bins bring none -- their key set
 * is the union of everything in their child IXF, computed on the device (a hash set in HBM), level by level from the leaves
 * up; the IXFs of one level share peeling chunks.  An IXF that does not peel is redone under a redrawn seed, it alone.
 * Unions are limited to 2^32 keys. */
int taxor_gpu_index_build_hixf(taxor_gpu_index *idx, const uint64_t *keys, const uint64_t *key_off, uint64_t seed0,
                               uint32_t *rounds_out);
/* The same two with the keys already ON THE INDEX'S DEVICE (keys_on_device != 0: `keys` is a device pointer; key_off
 * stays a host array) and with the run's figures. */
typedef struct taxor_build_stats {
    uint64_t keys_inserted;   /* key insertions done (a key below a merged bin counts once per level it is inserted at) */
    uint64_t scratch_bytes;   /* peeling scratch at its largest */
    uint32_t rounds_max;      /* peeling rounds of the slowest chunk */
    uint32_t reseeds;         /* IXFs redone under a new seed */
    uint32_t chunks;          /* peeling chunks */
    uint32_t reserved;
    double seconds_peel;      /* count + seed scan + rounds */
    double seconds_assign;    /* clearing, assignment in reverse, verification */
    double seconds_union;     /* duplicate-free unions of the merged bins' key sets */
    double seconds_total;     /* from the call to the last IXF built and verified (key upload and scratch allocation inside) */
    double seconds_release;   /* handing keys, unions and scratch back to the driver afterwards (not in seconds_total) */
    double seconds_count;     /* GPU time of k_count (3 atomic adds per key), HIP events on the builder's stream */
    double seconds_rounds;    /* GPU time of the seed scan and the peeling rounds (2 atomic subs per key), HIP events */
    double seconds_upload;    /* keys from host memory to the device (allocation + copy; 0 when they were there already); in seconds_total */
    double seconds_alloc;     /* hipMalloc / hipFree of the peeling scratch (in seconds_total; the driver's time, erratic for GB-sized blocks) */
    uint64_t keys_counted_in_lds; /* of keys_inserted: keys whose bin's degree words were built in LDS (no global atomic adds for them) */
    /* taxor_gpu_index_build_hixf_stream only (0 after any other build) */
    uint32_t stream_groups;   /* groups of IXFs whose keys were uploaded and built together */
    uint32_t stream_ranges;   /* bin ranges of an IXF larger than the budget (the last attempt's) */
    uint32_t stream_restarts; /* attempts of such an IXF thrown away because a bin did not peel under the seed */
    uint32_t reserved2;
    uint64_t stream_bytes_uploaded;       /* key bytes sent to the device, thrown-away attempts and unions read again included */
    double seconds_stream_upload;         /* ranged path: time the uploads of the bin ranges took (on their own thread and stream) */
    double seconds_stream_upload_wait;    /* of it: time the peeling waited for an upload (the rest was hidden behind peeling) */
} taxor_build_stats;
int taxor_gpu_index_build_ixf_ex(taxor_gpu_index *idx, uint64_t ixf, const uint64_t *keys, int keys_on_device,
                                 const uint64_t *key_off, uint64_t seed0, uint64_t *seed_out, taxor_build_stats *stats);
int taxor_gpu_index_build_hixf_ex(taxor_gpu_index *idx, const uint64_t *keys, int keys_on_device, const uint64_t *key_off,
                                  uint64_t seed0, taxor_build_stats *stats);
/* The same with GENERATED keys for some leaf bins: bin g (index bin order) holds gen_count[g] keys synth_key(gen_first[g] + k, gen_salt),
 * k < gen_count[g], instead of keys from `keys` (its key_off range is then empty).  Generated keys need no memory -- the kernels
 * compute them -- and a merged bin above an IXF of generated bins with consecutive index ranges is itself such a range, so an
 * index far larger than its keys would be (a 113-GB GTDB-class index has 7e10 of them: 560 GB) can be built with EVERY bin a
 * real filter.  Bins with real keys (planted genomes) and generated decoys mix freely. */
int taxor_gpu_index_build_hixf_gen(taxor_gpu_index *idx, const uint64_t *keys, int keys_on_device, const uint64_t *key_off,
                                   const uint64_t *gen_first, const uint64_t *gen_count, uint64_t gen_salt, uint64_t seed0,
                                   taxor_build_stats *stats);
/* ---- construction with the keys in HOST memory and a bounded part of them on the device ("Beyond device
 * memory").  The columns of an IXF are a function of its bins' key SETS and its seed alone, so what these build is byte-identical
 * to taxor_gpu_index_build_hixf on the same keys and seed0, whatever the budget.
 * taxor_gpu_keys_union: the duplicate-free union of n_lists key lists (host memory, or device memory with lists_on_device; the
 * lists need not be sorted nor free of duplicates themselves), with KeyUnion's device set (keyset.hip: its slot rule, and the
 * empty marker 2^64 - 1 kept aside and counted once).  *n_out = the union's exact size; with `out` != NULL the union itself, sorted
 * ascending, goes to out[0, *n_out) (device memory with out_on_device) -- TAXOR_E_ARG when out_cap is smaller. */
int taxor_gpu_keys_union(int device, const uint64_t *const *lists, const uint64_t *counts, uint64_t n_lists, int lists_on_device,
                         uint64_t *out, int out_on_device, uint64_t out_cap, uint64_t *n_out);
/* Bins [bin0, bin1) of one IXF under the seed GIVEN: no reseeding in here.  key_off[bins + 1] indexes `keys` for the IXF's bins
 * (only the entries bin0 .. bin1 are read); *ok = 1 when every bin of the range peeled and its columns are written, 0 when one did
 * not (nothing of this call is written then: the caller starts the IXF again from bin 0 under another seed).  flags:
 * TAXOR_BINS_CLEAR the whole IXF is set to 0 first (the first call of an attempt at an IXF all of whose bins have keys);
 * TAXOR_BINS_CLEARED it was, earlier in this attempt; neither: the range's columns are cleared one by one and bins without keys
 * keep their content.  A bin of 2^32 - 1 keys or more is TAXOR_E_ARG before anything is read.  On ok the index carries `seed`. */
#define TAXOR_BINS_CLEAR 1u
#define TAXOR_BINS_CLEARED 2u
int taxor_gpu_index_build_ixf_bins(taxor_gpu_index *idx, uint64_t ixf, uint64_t bin0, uint64_t bin1, const uint64_t *keys,
                                   int keys_on_device, const uint64_t *key_off, uint64_t seed, uint32_t flags, int *ok);
/* The whole hierarchy like taxor_gpu_index_build_hixf, with at most budget_bytes of keys on the device at a time: the IXFs of a
 * level in groups whose leaf keys and child unions fit the budget, every IXF's union written back to host memory for the level
 * above; an IXF whose own keys exceed the budget -- the root of a large index -- in bin ranges that fit, range r + 1 uploading into
 * a second buffer of the same size while range r peels, and from bin 0 again under the next seed when a bin does not peel (32
 * attempts).  TAXOR_E_ARG, naming it, for a child IXF whose keys alone exceed the budget and for a bin that does.  The peeling
 * scratch and the union table are the builder's own, beside the budget.
 * _ranges is the same with bin g's keys at host_keys[key_first[g], key_first[g] + key_count[g]): bins may lie in any order
 * (a build front end's store holds them in user bin order, the index wants them in its own). */
int taxor_gpu_index_build_hixf_stream(taxor_gpu_index *idx, const uint64_t *host_keys, const uint64_t *key_off, uint64_t seed0,
                                      uint64_t budget_bytes, taxor_build_stats *stats);
int taxor_gpu_index_build_hixf_stream_ranges(taxor_gpu_index *idx, const uint64_t *host_keys, const uint64_t *key_first,
                                             const uint64_t *key_count, uint64_t seed0, uint64_t budget_bytes, taxor_build_stats *stats);
/* Synthetic key sets for the build bench and tests: key i = a bijection of (i + salt) (distinct without a table);
 * taxor_gpu_synth_keys writes keys first .. first + n - 1 to the DEVICE array d_out, taxor_synth_key is the same
 * function on the host.  taxor_gpu_malloc / _free / _memcpy_to_host / _from_host: plain device memory for such arrays. */
uint64_t taxor_synth_key(uint64_t i, uint64_t salt);
int taxor_gpu_synth_keys(int device, uint64_t *d_out, uint64_t first, uint64_t n, uint64_t salt);
int taxor_gpu_malloc(int device, uint64_t bytes, void **out);
void taxor_gpu_free(void *p);
int taxor_gpu_memcpy_to_host(void *dst, const void *d_src, uint64_t bytes);
int taxor_gpu_memcpy_from_host(void *d_dst, const void *src, uint64_t bytes);

/* ---- `taxor build`: the key sets of whole reference genomes, on the device (taxor_amd/csrc/genome_keys.hip; the reference hashes
 * each genome file on a CPU thread, src/main/compute_hashes.cpp:50-142).  An accumulator: records arrive in any number of calls,
 * a user bin's records may span calls; _finish returns per user bin its DISTINCT keys, FracMinHash-filtered, sorted ascending:
 *   syncmers   union over the bin's records of hashing::seq_to_syncmers(k, record, s, t) (wyhash of canonical k-mers)
 *   minimisers union over its records of minimiser_hash(k, window_size, adjust_seed(k))
 *   scaling>1  only keys with double(wyhash(key)) <= double(UINT64_MAX) / scaling
 * Records are ASCII (any dna15 character; the dna4 mapping is applied on the device), at most 2^31 - 1 bases each. */
typedef struct {
    uint32_t kmer_size, syncmer_size, t_syncmer;
    uint32_t use_syncmer;     /* 1 = open canonical syncmers (s-mer sizes 1..31, as taxor_gpu_index_create admits), 0 = minimisers over window_size */
    uint64_t window_size;     /* minimiser mode: in [k, k+511] */
    uint32_t scaling;         /* > 1 = FracMinHash down-sampling */
    uint32_t reserved;
    uint64_t n_bins;          /* user bins; rec_bin values lie below it */
} taxor_keyer_params;
typedef struct {
    uint64_t calls, records, bases, tiles;
    uint64_t call_keys;       /* distinct keys summed over calls (a bin spread over calls counts in each) */
    uint64_t keys;            /* distinct keys after _finish */
    double seconds_device;    /* HIP-event time of packing, selection and set insertion, summed over calls */
    double seconds_add;       /* wall time inside _add (copies and per-call compaction included) */
    double seconds_finish;    /* wall time of _finish's gather, sort and merge */
} taxor_keyer_stats;
typedef struct taxor_gpu_keyer taxor_gpu_keyer;
int taxor_gpu_keyer_create(int device, const taxor_keyer_params *params, taxor_gpu_keyer **out);
/* records r < n_records: bases[rec_off[r] .. rec_off[r+1]) of user bin rec_bin[r] */
int taxor_gpu_keyer_add(taxor_gpu_keyer *kr, const char *bases, const uint64_t *rec_off, const uint32_t *rec_bin, uint64_t n_records);
/* CSR: keys of bin b at [bin_off[b], bin_off[b+1]), n_bins + 1 entries; *keys in host memory (may be NULL: not copied), *d_keys
 * the same on the keyer's device.  Valid until _destroy; no _add after _finish. */
int taxor_gpu_keyer_finish(taxor_gpu_keyer *kr, const uint64_t **bin_off, const uint64_t **keys, const uint64_t **d_keys);
/* exact number of distinct keys in the union of the listed user bins (a merged bin's key count), with KeyUnion's device set */
int taxor_gpu_keyer_union_size(taxor_gpu_keyer *kr, const uint32_t *bins, uint64_t n, uint64_t *out);
/* a new device array holding the finished keys' ranges [first[i], first[i] + count[i]) one after the other (the technical bins'
 * key lists in index order for taxor_gpu_index_build_hixf_ex); owned by the keyer, replaced by the next call */
int taxor_gpu_keyer_arrange(taxor_gpu_keyer *kr, const uint64_t *first, const uint64_t *count, uint64_t n_ranges, const uint64_t **d_out);
int taxor_gpu_keyer_stats(const taxor_gpu_keyer *kr, taxor_keyer_stats *out);
void taxor_gpu_keyer_destroy(taxor_gpu_keyer *kr);
/* free and total bytes of a device's memory */
int taxor_gpu_device_memory(int device, uint64_t *free_bytes, uint64_t *total_bytes);
/* The IXF tree of a build (host only; taxor_amd/csrc/host_util.cpp, DESIGN.md "taxor build"): from the distinct key count of every
 * user bin and t_max (0 = the candidates 64, 128, ..., 4096 and next_multiple_of_64(ceil(sqrt(n))) of taxor_build.cpp:173-187, the
 * one with the fewest expected fingerprint bytes gathered per query hash, then the fewest index bytes).  Every user bin is one run
 * of consecutive technical bins of one IXF (part j of parts of its sorted keys: [n*j/parts, n*(j+1)/parts)), no IXF has more than
 * t_max bins.  IXF 0 is the root; bins in index order: all of IXF 0, then IXF 1, ... */
typedef struct {
    uint64_t n_ixf, n_bins_total, t_max;
    uint32_t depth, reserved;
    double bytes_per_hash;      /* expected fingerprint bytes gathered per query hash (3 x stride along a user bin's path, weighted
                                   by the bins' key counts) */
    double index_bytes;         /* fingerprint bytes, merged bins counted as the sum of their children */
    const uint64_t *ixf_bins;   /* [n_ixf] */
    const uint64_t *bin_first;  /* [n_ixf + 1]: IXF i's bins are [bin_first[i], bin_first[i+1]) of the arrays below */
    const int64_t *next_ixf;    /* [n_bins_total] child IXF of a merged bin, the own IXF for a leaf */
    const int64_t *fname_idx;   /* [n_bins_total] user bin of a leaf, -1 = merged */
    const uint64_t *part;       /* [n_bins_total] leaf: which part of its user bin */
    const uint64_t *parts;      /* [n_bins_total] leaf: parts of its user bin; merged: 0 */
} taxor_layout;
int taxor_build_layout(const uint64_t *counts, uint64_t n, uint64_t t_max, taxor_layout **out);
void taxor_layout_free(taxor_layout *l);

/* ---- `taxor build --group-similar`: similar genomes under one merged bin (taxor_amd/csrc/sketch.hip, host_util.cpp; DESIGN.md
 * section 9, "Similarity-aware layout").
 * taxor_gpu_keys_sketch: bin b's keys are keys[off[b] .. off[b+1]) (host memory, or device memory with keys_on_device), distinct, as
 * taxor_gpu_keyer_finish delivers them.  sketch[b*m ..] receives the min(m, n_b) smallest values of mix(key), ascending, len[b] how
 * many; both in host memory, slots past len[b] unspecified.  mix is the fixed bijection of DESIGN.md.  m in [1, 1024].  Exact. */
int taxor_gpu_keys_sketch(int device, const uint64_t *keys, int keys_on_device, const uint64_t *off, uint64_t n_bins, uint32_t m,
                          uint64_t *sketch, uint32_t *len);
/* All pairs of n sketches, n in [1, 8192]; count[b] = keys of bin b, len[b] = min(count[b], m) (else TAXOR_E_ARG).  A sketch is
 * complete when count[b] <= m, then tau_b = 2^64 - 1, else tau_b is its largest value; tau = min(tau_a, tau_b);
 * shared[a*n + b] = values <= tau present in both sketches, uni[a*n + b] = |A <= tau| + |B <= tau| - shared.  kernel_ms (may be NULL)
 * receives the kernel's HIP-event time. */
int taxor_gpu_sketch_pairs(int device, const uint64_t *sketch, const uint32_t *len, const uint64_t *count, uint64_t n, uint32_t m,
                           uint32_t *shared, uint32_t *uni, float *kernel_ms);
/* Host only.  Rows i and j are linked when uni > 0 && (double)shared >= jmin * (double)uni; clusters are the connected components
 * (single linkage), ordered by their smallest member, members in ascending row order.  order[n]: that permutation of 0 .. n-1;
 * cluster[i] (may be NULL): the ordinal of row i's cluster. */
int taxor_cluster_order(const uint32_t *shared, const uint32_t *uni, uint64_t n, double jmin, uint64_t *order, uint64_t *cluster);
/* The global rank: the bins in descending key count (ties on index) are cut into consecutive windows of `window` bins (in [2, 8192]),
 * each window goes through taxor_gpu_sketch_pairs and taxor_cluster_order, and rank[u] is u's position in the concatenation of the
 * windows' orders.  sketch / len as taxor_gpu_keys_sketch left them for all n bins.  *n_multi (may be NULL): clusters with more than
 * one member; *pairs_ms (may be NULL): the pairs kernel's time summed over the windows. */
int taxor_similarity_rank(int device, const uint64_t *sketch, const uint32_t *len, const uint64_t *counts, uint64_t n, uint32_t m,
                          uint64_t window, double jmin, uint64_t *rank, uint64_t *n_multi, float *pairs_ms);
/* taxor_build_layout with one change: in every IXF the user bins that do not stay leaves are ordered by rank[u] (ascending; ties keep
 * the count order) instead of by count before they are cut into contiguous groups.  rank == NULL gives taxor_build_layout's result. */
int taxor_build_layout_ranked(const uint64_t *counts, uint64_t n, uint64_t t_max, const uint64_t *rank, taxor_layout **out);

/* ---- search of an index that does not fit the device ("Search beyond device memory").  A child IXF is reached
 * only through one merged bin of its parent, so the root stays resident and the SUBTREES -- one merged bin of the root with everything
 * below it -- are brought in group by group: every read is searched once per pass against "root + this pass's group", and per read the
 * passes' result lists are merged by DFS key.
 * taxor_index_plan_passes (host only, no HIP call): subtrees in root-bin order, packed greedily into groups.  Two groups are on the
 * device while one uploads behind the other, so root + group g + group g+1 <= budget_bytes for every g: a group is closed when the next
 * subtree would take it past HALF of what the root leaves (a larger subtree is a group of its own) or past what the group before it
 * leaves.  An index without a merged root bin, or one that fits the budget whole, is one pass.  Bytes are the slab's: every IXF rounded
 * up to 4 KiB, and the slab's 4-KiB tail pad counted with the root.  TAXOR_E_ARG with a named message (taxor_gpu_last_error) before any
 * work: "root-exceeds-budget" when the root alone exceeds the budget, "subtree-exceeds-budget" when one subtree exceeds what the root
 * (and the group before it) leaves -- that message names the root bin and the child IXF and says that a smaller --tmax at build time helps.
 * pass_of_ixf [n_ixf] (may be NULL): the pass an IXF is resident in, TAXOR_PASS_ROOT for the root; pass_bytes [n_ixf] (may be NULL): the
 * first n_passes entries receive the groups' bytes. */
#define TAXOR_PASS_ROOT 0xFFFFFFFFu
typedef struct {
    uint32_t n_passes, n_subtrees;
    uint64_t root_bytes;    /* root IXF + tail pad */
    uint64_t slab_bytes;    /* root_bytes + the largest pair of neighbouring groups: what a paged index allocates */
    uint64_t index_bytes;   /* root_bytes + every subtree */
} taxor_pass_plan;
int taxor_index_plan_passes(const taxor_hixf_view *view, uint64_t budget_bytes, taxor_pass_plan *plan, uint32_t *pass_of_ixf, uint64_t *pass_bytes);
/* An index whose slab is plan.slab_bytes <= budget_bytes: every table for the whole hierarchy, the root resident, every other IXF at a
 * fixed place of its group's half of the slab (even groups from the root upwards, odd groups from the end downwards), NO group loaded:
 * taxor_gpu_index_load_pass(idx, view, 0) comes before the first search.  taxor_gpu_index_data_bytes reports what is resident.  The
 * builders and taxor_gpu_index_download_ixf are not for such an index. */
int taxor_gpu_index_create_paged(const taxor_hixf_view *view, int device, uint64_t budget_bytes, taxor_gpu_index **out);
/* 0 for an ordinary index */
uint32_t taxor_gpu_index_passes(const taxor_gpu_index *idx);
/* Makes group `pass` the searched one: waits until it is resident (uploads it if nothing did), marks the children of every other
 * subtree absent -- a merged bin whose child is absent is counted and pruned as usual and nothing is enqueued for it -- and starts the
 * upload of group pass + 1 on a thread and streams of its own, into the half of the slab that pass - 1 used.  `view` is the one the
 * index was created from and stays valid until the next load_pass or the index's destruction.  pass is the one after the last loaded,
 * or 0 (start over); every search of the pass before must have ENDED (taxor_gpu_search_batch_end / _batch_sync) on every searcher of
 * the index: both are checked, TAXOR_E_ARG otherwise. */
int taxor_gpu_index_load_pass(taxor_gpu_index *idx, const taxor_hixf_view *view, uint32_t pass);
/* seconds taxor_gpu_index_load_pass has spent waiting for uploads so far (the rest of them was hidden behind the pass before) */
double taxor_gpu_index_upload_wait_seconds(const taxor_gpu_index *idx);
/* One earlier pass's results for the reads of the searcher's last batch, in host memory: the CSR as taxor_gpu_results gives it and the
 * tuples' DFS keys (taxor_gpu_results_keys). */
typedef struct {
    uint64_t n_reads, n_tuples;
    const uint64_t *read_off; /* [n_reads + 1] */
    const int64_t *user_bin;  /* [n_tuples] */
    const uint32_t *count;    /* [n_tuples] */
    const uint32_t *key;      /* [n_tuples] ascending within a read */
} taxor_gpu_prior;
/* After taxor_gpu_search_batch_end (or _batch_sync) of the LAST pass: merges, per read, the n_prior lists with the searcher's own by DFS
 * key on the device (one wavefront per read).  A key present in several lists is kept once -- a leaf bin of the root is found again in
 * every pass, with the same count; a differing count is TAXOR_E_INTERNAL.  Afterwards the searcher's device-resident CSR is the complete
 * one: taxor_gpu_batch_fetch, _batch_export_device, the communicator's gather and taxor_gpu_profile_feed_add_batch see it. */
int taxor_gpu_search_merge_prior(taxor_gpu_searcher *s, const taxor_gpu_prior *prior, uint32_t n_prior);
/* the DFS keys of the last results' tuples, [n_tuples] in host memory, valid until the next call on the searcher.  A call of a few
 * thousand reads keeps its keys only on a searcher of a paged index (TAXOR_E_ARG otherwise). */
int taxor_gpu_results_keys(taxor_gpu_searcher *s, const uint32_t **key);

/* ---- a batch's hash lists, saved once and replayed ("Search beyond device memory": capture and replay).  What the
 * query of a batch consumes -- every read's distinct hashes, their count and the read's threshold -- depends on the reads and on the
 * hashing and threshold parameters alone, not on which part of an index is resident: a caller that searches the same reads again (the
 * next pass over a paged index) keeps them and neither parses, uploads, packs nor hashes the reads a second time. */
typedef struct taxor_gpu_saved taxor_gpu_saved;
typedef struct {
    uint64_t n_reads, total_hashes, n_sub_batches;
    const uint32_t *read_len;    /* [n_reads] bases */
    const uint32_t *n_hashes;    /* [n_reads] distinct hashes (QHASH_COUNT) */
    const uint64_t *threshold;   /* [n_reads] the FINAL threshold, whatever the model: a replay evaluates none */
    const uint64_t *hash_off;    /* [n_reads + 1] read r's hashes are hashes[hash_off[r] .. hash_off[r+1]), first-insertion order */
    const uint64_t *hashes;      /* [total_hashes] dense, batch read order */
    const uint32_t *sub_first;   /* [n_sub_batches + 1] the run's sub-batch plan: reads [sub_first[i], sub_first[i+1]) were queried together */
    const uint32_t *order;       /* [n_reads] processing order inside each sub-batch (indices relative to its first read) */
    /* the searcher's hashing and threshold parameters at capture */
    uint32_t use_syncmer, kmer_size, syncmer_size, t_syncmer;
    uint32_t scaling, model;     /* model: TAXOR_THR_* */
    uint64_t window_size;        /* minimiser mode, else 0 */
    double error_rate, ratio;    /* ratio: the percentage / syncmer models' factor */
} taxor_gpu_saved_view;
/* on != 0: every batch the searcher runs from now on (taxor_gpu_search_batch, _batch_begin, _segments_begin, _nibbles_begin, _fastx_begin,
 * taxor_gpu_batch_run) also leaves a saved batch in host memory: per sub-batch, behind its hashing kernels, a scan of the counts and a
 * gather of the lists into a dense device array, copied out through a bounded page-locked buffer while the sub-batch is queried.  Calls
 * of a few thousand reads take the pipeline of large batches while capture is on (the lanes keep no hash lists).  on == 0: nothing of
 * this exists -- no launch, copy or allocation is added to any path -- and the capture's buffers are released. */
int taxor_gpu_search_capture(taxor_gpu_searcher *s, int on);
/* after taxor_gpu_search_batch_end (or _batch_sync) of a batch that ran with capture on: the saved batch, the caller's from then on
 * (taxor_gpu_saved_free).  TAXOR_E_ARG when capture is off or the batch was taken already. */
int taxor_gpu_search_take_saved(taxor_gpu_searcher *s, taxor_gpu_saved **saved);
/* read-only pointers into the saved batch, valid until it is freed; host bytes it holds */
int taxor_gpu_saved_view_get(const taxor_gpu_saved *saved, taxor_gpu_saved_view *view);
uint64_t taxor_gpu_saved_bytes(const taxor_gpu_saved *saved);
void taxor_gpu_saved_free(taxor_gpu_saved *saved);
/* ---- where along its read each saved hash lies.  Syncmer indexes only.  For read r of L bases, k-mer size k
 * and its list hashes[hash_off[r] .. hash_off[r+1]):
 *     pos[i] = min { p in [0, L-k] : wyhash_u64(min(f_p, revcomp(f_p))) == hashes[i] }
 * with f_p the 2-bit k-mer at base p of the packed read (after the dna4 mapping): the first base at which the read shows this k-mer, on
 * either strand.  It is defined by CONTENT: it equals the start of the window that first emitted the hash except where the reference's
 * stateful tie rule leaves a k-mer's first occurrence unselected and selects a later one -- pos is then the earlier occurrence, and
 * positions need not increase with i.  The same for FracMinHash-scaled lists (a subset).
 * on != 0, while capture is on: every batch from now on runs one more kernel per sub-batch behind the gather, on its stream
 * (k_hash_positions: the list in pieces of 2048 hashes in an LDS table, the read's k-mers swept once per piece), and its saved batch
 * carries a position store beside the hashes, 4 bytes per hash, copied out through a second bounded page-locked pair.  TAXOR_E_ARG, by
 * name: capture is off; a batch is in flight; the searcher does not hash syncmers (minimiser and k-mer lists are not deduplicated and
 * their values are not wyhash(k-mer)).  taxor_gpu_search_capture(s, 0) turns positions off as well.  A hash no k-mer of its read gives
 * is TAXOR_E_INTERNAL, naming the read; it is never a result.  A replay (taxor_gpu_search_saved_begin) ignores positions. */
int taxor_gpu_search_capture_positions(taxor_gpu_searcher *s, int on);
/* *pos: [total_hashes] parallel to the view's hashes, valid until the saved batch is freed; NULL when it was captured without
 * positions.  taxor_gpu_saved_bytes counts the store; taxor_gpu_saved_view is unchanged. */
int taxor_gpu_saved_positions(const taxor_gpu_saved *saved, const uint32_t **pos);
/* seconds between the event pairs around the batch's position kernels, one pair per sub-batch (0 without positions).  A sub-batch's
 * kernel runs beside the query of the sub-batch before it: this is the time it held its stream, not its time alone on the device. */
double taxor_gpu_saved_positions_seconds(const taxor_gpu_saved *saved);
/* The batch again, from its saved lists: they are staged sub-batch by sub-batch (same plan, same double buffering, same queue sizing as
 * the run from bases) and queried from level 0; nothing is packed or hashed.  taxor_gpu_search_batch_end follows, and afterwards the
 * searcher is where a batch from bases leaves it: taxor_gpu_batch_fetch, _batch_export_device, taxor_gpu_results_keys,
 * taxor_gpu_search_merge_prior, taxor_gpu_profile_feed_add_batch (the read lengths are on the device) and taxor_gpu_batch_stats work
 * unchanged.  `saved` stays valid until _batch_end.  The searcher may be another one and its index another index -- a paged index in
 * another pass is that case -- but its hashing and threshold parameters must be the saved batch's: TAXOR_E_ARG naming the field
 * (use_syncmer, kmer_size, syncmer_size, t_syncmer, window_size, scaling, model, error_rate, ratio) otherwise.  Before any launch the
 * host checks what the kernels rely on (TAXOR_E_ARG naming the field): hash_off ascending from 0 and inside the array, n_hashes
 * consistent with it, sub_first tiling the reads, order inside its sub-batch. */
int taxor_gpu_search_saved_begin(taxor_gpu_searcher *s, const taxor_gpu_saved *saved);
/* Host only: host bytes the saved hash lists of `bases` bases of query may need -- 8 per hash at one hash per min(t, k-s+1-t+1) bases
 * for syncmers (k22/s12/t5: per 5 bases), per base otherwise, plus one per k bases, and 28 per read at one read per 200 bases -- and
 * whether a store of that bound fits `available_bytes` with a quarter of a gibibyte to spare (1; always 1 when available_bytes is 0:
 * no figure to hold against).  `taxor search` decides between replaying and re-reading the query with these two. */
uint64_t taxor_saved_bytes_bound(uint64_t bases, int use_syncmer, uint32_t kmer_size, uint32_t syncmer_size, uint32_t t_syncmer);
int taxor_saved_store_fits(uint64_t bound_bytes, uint64_t available_bytes);

/* ---- taxor_gpu_search_batch split into its three phases so that a caller can keep a batch resident in HBM
 * (upload once, run many times) and overlap transfers with compute:
 *   upload : H2D of the ASCII bases + on-device dna4 mapping and 2-bit packing
 *   run    : all kernels (syncmers -> dedup -> threshold -> level-synchronous HIXF query -> DFS order),
 *            asynchronous on the searcher's stream
 *   fetch  : wait + D2H of the CSR results */
int taxor_gpu_batch_upload(taxor_gpu_searcher *s, const char *bases, const uint64_t *offsets,
                           uint64_t n_reads);
/* taxor_gpu_batch_upload with the HIP-event time of its packing kernel (k_pack_dna4) in *kernel_ms: the figure that stands beside
 * taxor_gpu_pack_nibbles' kernel_ms in measurements */
int taxor_gpu_pack_dna4_timed(taxor_gpu_searcher *s, const char *bases, const uint64_t *offsets, uint64_t n_reads, float *kernel_ms);
int taxor_gpu_batch_run(taxor_gpu_searcher *s);
int taxor_gpu_batch_sync(taxor_gpu_searcher *s);
int taxor_gpu_batch_fetch(taxor_gpu_searcher *s, taxor_gpu_results *out);
/* Device-resident results of the last run (for an RCCL gather): sizes, then D2D copy into caller-provided
 * DEVICE buffers (read_off u64[n_reads+1], user_bin i64[n_tuples], count u32[n_tuples], n_hashes
 * u32[n_reads]); any pointer may be NULL to skip it.  Synchronises the searcher's stream. */
int taxor_gpu_batch_result_sizes(taxor_gpu_searcher *s, uint64_t *n_reads, uint64_t *n_tuples);
int taxor_gpu_batch_export_device(taxor_gpu_searcher *s, void *d_read_off, void *d_user_bin, void *d_count,
                                  void *d_n_hashes);


/* ---- communicator statistics and the one-GPU test hook */
typedef struct {
    int32_t transport;
    uint32_t n_devices;
    uint64_t index_bytes;            /* fingerprint bytes of one replica                                  */
    uint64_t index_upload_bytes;     /* bytes that crossed PCIe host -> device for the replicas           */
    uint64_t index_broadcast_bytes;  /* bytes delivered device -> device by ncclBroadcast                 */
    double index_seconds;            /* wall time of taxor_gpu_index_create_replicated                    */
    uint64_t gathers, gather_bytes;  /* gather calls; result bytes that left a peer device                */
    double gather_seconds;           /* wall time inside taxor_gpu_gather_results (sync of the runs included) */
    uint64_t index_broadcast_calls;  /* grouped ncclBroadcast rounds issued behind the upload (RCCL transport)  */
    uint64_t self_exchange_bytes;    /* result bytes rank 0 sent to itself through ncclSend/ncclRecv (test hook below) */
    int32_t rccl_version;            /* ncclGetVersion of the RCCL bound at run time, 0 = none loaded           */
    uint64_t selftest_bytes;         /* known bytes verified through ncclBroadcast + ncclSend/ncclRecv at creation (RCCL) */
} taxor_gpu_comm_stats;
int taxor_gpu_comm_info(const taxor_gpu_comm *c, taxor_gpu_comm_stats *out);
/* Test hook for boxes with ONE GPU: with on != 0, rank 0's own part of every gather travels through the grouped
 * ncclSend / ncclRecv (to itself) like a peer's instead of a device-to-device copy, so a communicator of one rank executes
 * the exchange code of a larger run line by line.  Results are unchanged.  RCCL transport only. */
int taxor_gpu_comm_set_self_exchange(taxor_gpu_comm *c, int on);

/* Measurement of the last taxor_gpu_batch_run (valid after sync).  algorithmic_bytes follows SURVEY.md
 * section 8(d): sum over reads of ceil(L/4) + sum over visited IXFs n_h*3*bins + 8 + 12*tuples;
 * query_* are the dominant kernel (k_query_level) only: launches, HIP-event milliseconds on the searcher's
 * stream (0 unless time_kernels), and its gather bytes sum n_h*3*bins. */
typedef struct {
    uint64_t n_reads, n_bases, n_hashes, n_tuples, n_work_items;
    uint64_t algorithmic_bytes;
    uint64_t query_bytes;
    uint64_t query_touched_bytes; /* bytes k_query_level actually requested: threshold-aware pruning skips row
                                     segments of bin runs that provably cannot reach the threshold       */
    uint32_t query_launches;
    float query_ms;
    float syncmer_ms;
    float finalize_ms;
    float total_ms;
    /* k_query_level per HIXF level (level 7 collects everything deeper): HIP-event milliseconds, requested bytes, and
     * fingerprint-row reads (levels of rows <= 128 B are bound by DRAM row activations, not by bytes) */
    float level_ms[8];
    uint64_t level_requested_bytes[8];
    uint64_t level_row_reads[8];
    uint64_t level_sparse_loads[8];  /* of level_row_reads: 16-B loads of the pruned (sparse) phase, one fingerprint row each;
                                        level_requested_bytes bills each as one 64-B sector */
    uint32_t tree_stalls_recovered;  /* pieces of a small call whose one-launch traversal gave up waiting (its watchdog fired) and
                                        were classified again level by level; results are unaffected */
    uint32_t small_pieces_rerun;     /* pieces of a small call that were classified again through the pipeline of large batches, for
                                        any reason (a queue, the hit buffer or the result area too small, or a stall as above);
                                        0 says that every piece of the call was assembled by the lanes' own finalize */
    uint64_t screen_plane_loads;     /* rows of the root's 2-bit plane read by the screen of large batches (three per screened hash); they
                                        are in level_requested_bytes[0] with their bytes and in level_row_reads[0] as the fraction of a
                                        full row that a plane row is.  0: nothing was screened */
} taxor_gpu_run_stats;
/* The root's 2-bit plane (a quarter-size copy of the root's rows holding fingerprint & 3, 16 bins per 32-bit word, low bins first;
 * derived on the device, never stored): *rows and *plane_stride as the searches see it, both 0 when the root has none; with out != NULL
 * (len = rows * plane_stride) the plane itself, derived first if the root was written since. */
int taxor_gpu_index_root_plane(taxor_gpu_index *idx, uint8_t *out, uint64_t len, uint64_t *rows, uint32_t *plane_stride);
int taxor_gpu_batch_stats(taxor_gpu_searcher *s, taxor_gpu_run_stats *out);
/* Measurement aid: a searcher created while TAXOR_PROFILE_PHASES=1 is set launches instrumented instantiations of the
 * two big kernels (s_memtime marks at their phase boundaries, summed over blocks).  Returns and clears 16 cycle sums:
 * [0..7] k_syncmers (cursor, staging, s-mer values, window argmins, selection, hash emit, dedup, copy-out),
 * [8..15] k_query_level (cursor+flush, metadata+probe staging, dense gathers, prune check, sparse gathers, tally,
 * final flush, -).  Results are unchanged; throughput is not (the marks cost a few percent). */
int taxor_gpu_phase_profile(taxor_gpu_searcher *s, uint64_t *cycles16);

/* ------------------------------------------------------------------------------------------------
 * Stage entry points (used by the parity tests; each stage is checked on its own against the oracle).
 * ---------------------------------------------------------------------------------------------- */
/* hashing::seq_to_syncmers (src/hashing/syncmer.hpp:23) for a batch: distinct hashes of read r, in first-
 * insertion order, at hashes[hash_off[r] .. hash_off[r+1]) -- after the FracMinHash filter of
 * taxor_search.cpp:223-233 when the index has scaling > 1.  Pointers valid until the next call. */
int taxor_gpu_syncmers(taxor_gpu_searcher *s, const char *bases, const uint64_t *offsets, uint64_t n_reads,
                       const uint64_t **hash_off, const uint64_t **hashes);
/* ixf.counting_agent<uint32_t>().bulk_count(values) for one IXF of the index
 * (call site hierarchical_interleaved_xor_filter.hpp:307-309): counts[bins]. */
int taxor_gpu_ixf_bulk_count(taxor_gpu_searcher *s, uint64_t ixf, const uint64_t *hashes, uint64_t n,
                             uint32_t *counts);
/* membership_agent::bulk_contains(values, threshold) (:381-406) for one hash list. */
int taxor_gpu_bulk_contains(taxor_gpu_searcher *s, const uint64_t *hashes, uint64_t n, uint64_t threshold,
                            taxor_gpu_results *out);
/* k_pack_nibbles alone (taxor_amd/csrc/bam_pack.hip; the segments are those of taxor_gpu_search_nibbles_begin, described there): the
 * packed words in host memory, read r's at words[word_off[r] .. word_off[r+1]) -- 16 bases per word, the first in the top bits, a
 * read's words padded with zeros to a multiple of four: what taxor_gpu_batch_upload leaves on the device.  kernel_ms (may be NULL)
 * receives the kernel's HIP-event time.  Pointers valid until the next call on the searcher. */
typedef struct {
    const uint8_t *seq4;
    const uint64_t *byte_off;   /* [n_reads] ascending */
    const uint32_t *read_len;   /* [n_reads] bases */
    const uint8_t *reverse;     /* [n_reads] or NULL */
    uint64_t n_reads;
} taxor_nibble_segment;
int taxor_gpu_pack_nibbles(taxor_gpu_searcher *s, const taxor_nibble_segment *segs, uint64_t n_segs, const uint64_t **word_off,
                           const uint32_t **words, float *kernel_ms);


/* ---- Diagnosis of an index this library did not write (`taxor verify --variants`, `taxor pin`).  Both the
 * arithmetic of seqan3::interleaved_xor_filter and the way its serialiser lays the fingerprints out are un-vendored in the
 * reference; taxor_amd/csrc/ixf_arith.h holds this library's reading of the former (evidence: src/main/xorfilter.hpp:36-45,
 * 60-68,338-350, src/main/hashutil.hpp:50-61), taxor_amd/csrc/ixf_layout.h the layouts a file may follow.  A variant is one
 * reading of the same RAW bytes; the scan probes one IXF's raw bytes under every variant with hash lists cut from sequences that
 * are in the index and reports, per (variant, list), the best-bin match ratio: ~1.0 under the file's true reading, ~2^-8
 * otherwise.  best_ratio[n_variants * n_lists], variant-major. */
typedef struct {
    uint64_t seed;
    uint64_t seg_len;   /* rows per hash segment */
    uint64_t stride;    /* the source's row pitch in bytes (row-interleaved) / bin columns stored (bin-major); unused for bit-sliced */
    uint8_t key_hash;   /* 0 murmur64 finaliser (hashutil.hpp:50-57), 1 none, 2 wyhash mix, 3 splitmix64 finaliser */
    uint8_t seed_mode;  /* 0 h(key + seed) (hashutil.hpp:59-61), 1 h(key ^ seed), 2 h(key) + seed, 3 seed unused */
    uint8_t rot;        /* row i uses rotl64(h, rot * i); 21 in xorfilter.hpp:42-45 */
    uint8_t reduce;     /* 0 ((u32)rot * seg_len) >> 32 (xorfilter.hpp:36-40), 1 (u32)rot % seg_len, 2 mulhi64(rot, seg_len) */
    uint8_t fp_mode;    /* 0 (u8)(h ^ h>>32) (xorfilter.hpp:60-62), 1 (u8)h, 2 (u8)(h>>56), 3 (u8)(h>>32) */
    uint8_t pad;
    uint16_t layout;    /* layout code (taxor_hixf_view::ixf_layout): kind and row order; the pitch bits say how `stride` was
                           derived (0 bins padded to 64, 1 exactly bins, 2 the record's stored scalar) */
} taxor_ixf_variant;
/* The arithmetic part of a variant (key hash, seed entry, rotation step, range reduction, fingerprint fold) as the code an index
 * carries (taxor_hixf_view::ixf_arith); 0 for this library's reading.  _decode fills those five fields and leaves the others. */
uint32_t taxor_ixf_arith_code(const taxor_ixf_variant *v);
void taxor_ixf_arith_decode(uint32_t code, taxor_ixf_variant *out);
/* this library's reading for the given seed / segment length / stride */
void taxor_ixf_variant_default(taxor_ixf_variant *out, uint64_t seed, uint64_t seg_len, uint64_t stride);
/* raw = the IXF's bytes as the file holds them (host memory, e.g. taxor_hixf_get_view()->ixf[i].data), raw_len of them */
int taxor_gpu_ixf_variant_scan(int device, const uint8_t *raw, uint64_t raw_len, uint64_t bins, const taxor_ixf_variant *variants,
                               uint32_t n_variants, const uint64_t *hashes, const uint64_t *hash_off, uint64_t n_lists, float *best_ratio);
/* one-line description of a variant; returns the length written */
uint64_t taxor_ixf_variant_describe(const taxor_ixf_variant *v, char *buf, uint64_t cap);
/* "bin-major,unpadded,position-major" <-> layout code; tokens: interleaved | bin-major | bit-sliced, padded | unpadded |
 * stored-pitch, segment-major | position-major; what is left out keeps the search layout's choice.  _parse returns 0 or TAXOR_E_ARG */
int taxor_ixf_layout_parse(const char *spec, uint32_t *code);
uint64_t taxor_ixf_layout_describe(uint32_t code, char *buf, uint64_t cap);

/* ---- .hixf: the record of one seqan3::interleaved_xor_filter inside the file (UN-VENDORED in the reference; this library's own
 * is documented in taxor_amd/csrc/hixf_io.cpp): n_before u64 scalars, the fingerprint vector (u64 length + bytes), n_after u64
 * scalars.  idx_* select the scalar (counted over before-then-after) that holds a field, -1 = not stored: bins then come from
 * next_ixf_id's inner sizes, the pitch from the layout's rule, seg_len = rows / 3, seed = default_seed. */
typedef struct {
    uint32_t n_before, n_after;
    int32_t idx_bins, idx_stride, idx_seg_len, idx_seed;
    uint32_t seg_len_is_rows;   /* 1: the idx_seg_len scalar holds rows = 3*seg_len */
    uint64_t default_seed;      /* 13572355802537770549 = the fixed start seed of src/main/xorfilter.hpp:153 */
    uint32_t layout;            /* how the fingerprint vector is laid out (taxor_hixf_view::ixf_layout); 0 = the search layout */
    uint32_t len_unit;          /* what the vector's u64 length word counts: 0 / 1 bytes (cereal's std::vector<uint8_t>), 8 = 64-bit words
                                   (std::vector<uint64_t>), 64 = BITS held in whole 64-bit words (an sdsl int_vector / bit_vector) */
    uint32_t skip_before_len, skip_after_len; /* bytes between the scalars and the length word / between it and the data (an int_vector's
                                   u8 width); the scalars themselves are u64 */
} taxor_ixf_schema;
/* this library's own schema: bins | technical_bins | seg_len | bin_words | seed | ftype | data, layout 0 */
void taxor_ixf_schema_default(taxor_ixf_schema *out);
/* `hixf-probe`: walk a real file with every (n_before, n_after) until the records re-parse n times and the pinned tail
 * (next_ixf_id, user_bins) lands exactly on end-of-file, then infer which scalar is which and which layouts the array lengths
 * admit (the layout itself is decided by the variant scan).  Writes a human-readable report (NUL-terminated, truncated to cap). */
int taxor_hixf_probe(const char *path, taxor_ixf_schema *out, char *report, uint64_t cap);
int taxor_hixf_load_schema(const char *path, const taxor_ixf_schema *schema, taxor_hixf **out);
/* writes view's IXFs (host bytes in the SEARCH layout, view->ixf_layout == 0) under schema->layout: what another writer's file
 * would look like (tests of the re-layout; export) */
int taxor_hixf_store_schema(const char *path, const taxor_hixf_view *view, const taxor_hixf_meta *meta, const taxor_ixf_schema *schema);
/* bytes of IXF i's fingerprint vector as the file holds it */
uint64_t taxor_hixf_ixf_raw_bytes(const taxor_hixf *h, uint64_t ixf);

/* ---- host-side XOR-filter construction and the synthetic workload */
/* seg_len of an IXF sized for max_bin_elements keys per bin: (size_t)(32 + 1.23*n) / 3 */
uint64_t taxor_ixf_seg_len(uint64_t max_bin_elements);
/* XOR-filter construction of one bin column (3*seg_len bytes) for `keys` under (seed, seg_len); returns 0,
 * or 1 if peeling failed for this seed (caller redraws the seed like construct_ixf.cpp:100-108). */
int taxor_ixf_build_bin(const uint64_t *keys, uint64_t n, uint64_t seed, uint64_t seg_len, uint8_t *column);
/* the same under another arithmetic code (taxor_ixf_arith_code) */
int taxor_ixf_build_bin_arith(const uint64_t *keys, uint64_t n, uint64_t seed, uint64_t seg_len, uint32_t arith, uint8_t *column);
/* Seeded synthetic long reads: read i is drawn from genome g_i at a uniform start
 * (reverse-complemented with probability frac_reverse) with ONT-like errors at rate e (40/30/30
 * sub/ins/del), or uniformly random with probability frac_random.  Note: with the reference's
 * t = ceil((k-s+1)/2) in INTEGER division (taxor_build.cpp:509-510; 5 at k22/s12) open-syncmer selection
 * is not strand-symmetric, so a reverse-strand read shares no syncmers with a forward-indexed genome.  genomes = concatenated ACGT, genome_off[n_genomes+1].  Writes ASCII into bases (capacity
 * cap) and offsets[n_reads+1]; origin[i] = genome index or -1.  Deterministic in (seed, i). */
int taxor_synth_reads(const char *genomes, const uint64_t *genome_off, uint64_t n_genomes, uint64_t n_reads,
                      uint32_t read_len, double error_rate, double frac_random, double frac_reverse,
                      uint64_t seed, int threads, char *bases, uint64_t cap, uint64_t *offsets, int32_t *origin);

/* ---- `taxor profile` (src/main/taxor_profile.cpp) over a CSR read -> matches; taxor_amd/csrc/profile.hip, DESIGN.md section 10.
 * Reads and references are numbered in byte-wise order of their names (the reference iterates std::map<std::string, ...>, and
 * that order is observable); a read's matches stand in file order.  A read without a hit has ONE match with ref -1 (the "-"
 * line).  A match never moves: the stages keep an alive byte per match. */
typedef struct taxor_gpu_profile taxor_gpu_profile;
typedef struct {
    uint64_t n_reads, n_refs, n_matches;
    const uint64_t *read_off;    /* [n_reads + 1] */
    const int32_t *ref;          /* [n_matches] reference id, -1 for the "-" line */
    const uint64_t *ref_len;     /* [n_matches] */
    const uint64_t *hash_match;  /* [n_matches] QUERY_HASH_MATCH */
    const uint64_t *query_len;   /* [n_reads] */
    const uint64_t *hash_count;  /* [n_reads] QUERY_HASH_COUNT */
} taxor_profile_csr;
#define TAXOR_PROFILE_TRACE 1u   /* keep the per-stage and per-iteration outputs the stage tests compare */
typedef struct {
    uint64_t n_reads, n_refs, n_matches;
    const int32_t *ref;          /* [n_matches] after round 3's renames */
    const uint64_t *ref_len;     /* [n_matches] likewise */
    const uint8_t *alive;        /* [n_matches] after the EM's erasures; a read is reported iff one of its matches is alive */
    const uint8_t *best;         /* [n_matches] the last iteration's best matches (profile_results) */
    const uint8_t *has_prior;    /* [n_refs] the found taxa: seen in round 3 and explained by no other reference */
    const uint64_t *taxa_len;    /* [n_refs] ref_len of the reference's first match in round 3 */
    const uint64_t *ref_nts;     /* [n_refs] nucleotides of the reads whose best set holds the reference, last iteration */
    const double *log_prior;     /* [n_refs] log sequence abundance after the last update */
    const int32_t *explained_by; /* [n_refs] the reference that explains this one, after chain resolution, or -1 */
    const uint32_t *unique_reads, *all_reads;   /* [n_refs] round 3's unique_assign_reads / all_assigned_reads */
    uint64_t all_nts, unclassified_nts;
    double log_unclassified;
    uint32_t em_steps_needed;    /* what the reference prints as "Number of EM steps needed" */
    uint32_t em_iterations;      /* passes of the loop body */
    uint64_t n_pairs, pair_slots;   /* occupied slots / slots of the pair table */
    const uint64_t *pair_key;    /* [n_pairs] ref1 << 32 | ref2, in table order */
    const uint32_t *pair_count;  /* [n_pairs] reads the two share */
    /* with TAXOR_PROFILE_TRACE, else null: alive after each round, ref_nts of every iteration [em_iterations * n_refs] */
    const uint8_t *alive_round1, *alive_round2, *alive_round3;
    const uint64_t *iter_ref_nts;
    double seconds_filter, seconds_em;
} taxor_profile_results;
int taxor_gpu_profile_create(int device, const taxor_profile_csr *csr, taxor_gpu_profile **out);
/* the three rounds and at most em_steps EM iterations; once per object.  TAXOR_E_ARG with a message that names the situation for
 * the two inputs the reference leaves undefined: an explained-by chain that runs into a cycle, and a multi-match read none of
 * whose references has a prior */
int taxor_gpu_profile_run(taxor_gpu_profile *p, uint32_t em_steps, uint32_t flags);
/* pointers stay valid until _destroy */
int taxor_gpu_profile_results(taxor_gpu_profile *p, taxor_profile_results *out);
void taxor_gpu_profile_destroy(taxor_gpu_profile *p);

/* ---- search -> profile without the TSV (taxor_amd/csrc/profile_feed.hip): a feed on one device collects,
 * batch by batch and in any order, the read -> matches CSR that taxor_gpu_profile_create takes from the host.  ref_of_bin[u] is the
 * dense id of user bin u's accession (ids in byte-wise order of the distinct accession strings; user bins of one accession share an
 * id), ref_len_of_bin[u] its species' seq_len.  flags 0 applies the search's output filter (taxor_search.cpp:268-306: a tuple is
 * dropped iff (double)count < (double)max_count * 0.8; a read that keeps nothing is ONE match with ref -1 and QHASH_COUNT 0);
 * TAXOR_FEED_KEEP_ALL appends every tuple (rows that passed the filter already).  A batch is never truncated: the stores grow.
 * _add calls may come from several threads. */
typedef struct taxor_gpu_profile_feed taxor_gpu_profile_feed;
#define TAXOR_FEED_KEEP_ALL 1u
int taxor_gpu_profile_feed_create(int device, uint64_t n_user_bins, const int32_t *ref_of_bin, const uint64_t *ref_len_of_bin, uint64_t n_refs,
                                  taxor_gpu_profile_feed **out);
/* the results of the searcher's last run where they lie on the feed's device (the buffers taxor_gpu_batch_export_device copies
 * from; QUERY_LEN from the batch's offsets); first_read = index of the batch's first read among all reads.  Waits for the run; when
 * it returns the searcher may run again */
int taxor_gpu_profile_feed_add_batch(taxor_gpu_profile_feed *f, taxor_gpu_searcher *s, uint64_t first_read, uint32_t flags);
/* the same over host arrays: tuples of read r at [read_off[r], read_off[r+1]) of user_bin / count, n_hashes and query_len [n_reads] */
int taxor_gpu_profile_feed_add_csr(taxor_gpu_profile_feed *f, uint64_t first_read, uint64_t n_reads, const uint64_t *read_off, const int64_t *user_bin,
                                   const uint32_t *count, const uint32_t *n_hashes, const uint64_t *query_len, uint32_t flags);
/* rank_of_read[i] = position of read i in byte-wise order of the read ids.  Permutes the CSR into that order on the device and
 * hands the device arrays to a new taxor_gpu_profile (_run, _results, _destroy as above; the caller destroys it).  TAXOR_E_ARG
 * unless the batches' ranges cover [0, n_reads_total) exactly once and the ranks are a permutation */
int taxor_gpu_profile_feed_finish(taxor_gpu_profile_feed *f, const uint64_t *rank_of_read, uint64_t n_reads_total, taxor_gpu_profile **profile);
/* after _finish: the finished CSR (reads in rank order) in host memory, and per match the user bin it came from (-1 for the "-"
 * match) -- a binning file prints the taxid of the ORIGINAL line.  Either pointer may be NULL.  Valid until _destroy */
int taxor_gpu_profile_feed_matches(const taxor_gpu_profile_feed *f, taxor_profile_csr *csr, const int64_t **user_bin);
void taxor_gpu_profile_feed_destroy(taxor_gpu_profile_feed *f);

/* ---- distinct matched hashes per reference (`taxor search --coverage-file`; taxor_amd/csrc/coverage.hip, DESIGN.md section 10,
 * "Distinct-hash coverage").  QHASH_MATCH summed over reads grows with depth whether the hits spread over a genome or pile up on one
 * repeat; the accumulator keeps, per user bin and for the whole run, a HyperLogLog sketch of the DISTINCT query hashes that matched it,
 * beside the number of reads that reported it and the sum of their counts.
 * A (read, user bin) pair counts when the read's tuple for that bin survives the search's output filter -- taxor_classify_filter's
 * !((double)count < (double)max * 0.8) -- so reads[b] and hash_matches[b] are what one gets by counting and summing the TSV's lines of
 * user bin b.  For such a pair every hash h of the read's saved list is looked up in every leaf technical bin (x, j) of b (each bin
 * with fname_idx == b anywhere in the hierarchy; a split user bin has several): h matches when the three fingerprints of IXF x at h's
 * rows in column j xor to h's fingerprint, under the index's arithmetic code and x's seed.  A hash that matches in at least one of
 * them goes into b's sketch: (i, rho) = taxor_hll_slot(h, P), registers[b][i] = max(registers[b][i], rho).
 * _create: precision P in [4, 16], 0 = 12; `view` is the one the index was created from (only bins and fname_idx are read).  The
 * registers (n_user_bins << P bytes) and the two counters are held against the device's free memory first: TAXOR_E_NOMEM with both
 * figures.  A paged index is refused by name (TAXOR_E_ARG): its leaf bins are not all resident.
 * _add_batch: after taxor_gpu_search_batch_end (or _batch_sync) of a batch that ran with capture on, with that batch's saved lists
 * (taxor_gpu_search_take_saved), before the next batch on the searcher.  Checked before any launch, TAXOR_E_ARG naming the field:
 * the saved batch's n_reads is the searcher's, its n_hashes are the searcher's, the searcher's index is the accumulator's.  The lists
 * are staged through a bounded device buffer; the searcher's device-resident CSR is read where it lies.  Calls may come from
 * several threads.  The result does not depend on the order of the calls nor on how reads are cut into batches.
 * _results: host pointers, valid until _destroy or the next _add_batch. */
typedef struct taxor_gpu_coverage taxor_gpu_coverage;
typedef struct {
    uint64_t n_user_bins;
    uint32_t precision, reserved;
    const uint64_t *reads;         /* [n_user_bins] surviving tuples of the user bin (lines of the TSV) */
    const uint64_t *hash_matches;  /* [n_user_bins] their counts summed (QHASH_MATCH summed) */
    const uint8_t *registers;      /* [n_user_bins << precision] user bin b's sketch at registers + (b << precision) */
    double seconds_kernels;        /* HIP-event time of the accumulation kernel, summed over the batches */
    uint64_t probes;               /* (hash, leaf bin) lookups made: three one-byte gathers each */
} taxor_coverage_results;
int taxor_gpu_coverage_create(taxor_gpu_index *idx, const taxor_hixf_view *view, uint32_t precision, taxor_gpu_coverage **out);
int taxor_gpu_coverage_add_batch(taxor_gpu_coverage *c, taxor_gpu_searcher *s, const taxor_gpu_saved *saved);
int taxor_gpu_coverage_results(taxor_gpu_coverage *c, taxor_coverage_results *out);
void taxor_gpu_coverage_destroy(taxor_gpu_coverage *c);
/* Host only.  The slot of a hash: w = wyhash(hash ^ 0x9E3779B97F4A7C15), index = w >> (64 - P), rest = w << P,
 * rho = rest ? clz64(rest) + 1 : 64 - P + 1 -- the function the device uses (taxor_amd/csrc/hll.h).  The estimate: m = 2^P,
 * alpha = 0.673, 0.697, 0.709 for m = 16, 32, 64, else 0.7213 / (1 + 1.079 / m); E = alpha m^2 / sum_j 2^-registers[j] in index
 * order; E = m log(m / V) when E <= 2.5 m and V > 0 registers are zero; no large-range correction (the hashes are 64-bit).  A
 * precision outside [4, 16]: index 0 and rho 0, NaN. */
double taxor_hll_estimate(const uint8_t *registers, uint32_t precision);
void taxor_hll_slot(uint64_t hash, uint32_t precision, uint32_t *index, uint8_t *rho);

/* ---- per-read lowest common ancestor and per-taxon tallies (`taxor search --lca-file / --report-file`; taxor_amd/csrc/lineage.h and
 * lca.hip).
 * The lineage (host only).  User bin b's species is the first species whose user_bin == b, species[0] if there is none
 * (taxor_format_read's rule).  ids = split(taxid_string, ';'), names = split(taxnames_string, ';'), no trailing empty field; position d
 * of ids pairs with position d of names.  A node is a distinct non-empty id string; node numbers are dense, in byte-wise order of the
 * id strings.  A node's name is names[d] without its first three characters (empty if shorter than 3), its rank letter names[d][0]
 * ('-' if the field is empty); the first occurrence in user-bin order decides.  The compacted path of b is its non-empty ids as node
 * numbers, root-down; a node's parent is its predecessor, the first node's parent is ROOT.  ROOT is a virtual node with id string "1",
 * name "root", rank 'R'; a compacted path whose first id is "1" starts at ROOT itself, and that id is not stored in path[].  Refused
 * (TAXOR_E_ARG, the message names the ids and the accessions): an id with two different parents in two paths, an id twice in one path
 * (a "1" anywhere but first included), a compacted path of more than 64 ids (a leading "1" counts), names shorter than ids.  A user bin
 * without a non-empty id has the empty path and sits directly under ROOT.
 * The accumulator lives beside a resident index for a whole run.  _create uploads the paths as a CSR (path_off, path): real paths
 * hold seven or eight nodes, and a fixed pitch of the maximum depth would let ONE deep path multiply the table of every user bin by up
 * to eight; the CSR costs one more 4-byte load per surviving tuple.  It allocates direct_reads and direct_bases, 64-bit, for the nodes
 * plus ROOT plus UNCLASSIFIED.  TAXOR_E_ARG naming the field: the lineage's n_user_bins is not the index's; a paged index is refused by
 * name (its final tuples exist only after the last pass's merge).
 * For read r with tuples T: m = the maximum count; the survivors are the tuples with !((double)count < (double)m * 0.8), fp64 as
 * written (taxor_classify_filter's expression).  T empty or m == 0: UNCLASSIFIED, n_refs = 0, best = 0 -- a read without a hash
 * reports every leaf with count 0 and the TSV prints those lines; here nothing matched, so the read is unclassified.  Otherwise node =
 * the last node of the longest common prefix of the survivors' compacted paths, ROOT for the empty prefix; best = m; n_refs = the
 * survivors.  direct_reads[node] += 1, direct_bases[node] += the read's length.
 * _add_batch: after taxor_gpu_search_batch_end (or _batch_sync), before the next batch on the searcher.  Reads the searcher's
 * device-resident CSR where it lies, the read lengths from the batch's offsets; one kernel (one wave per read).  No capture is needed.
 * calls: page-locked host memory, valid until the next _add_batch on THAT searcher (or _destroy); n_hashes is the searcher's QHASH_COUNT
 * per read, copied beside the three words of the call.  first_read numbers the batch's first read among all reads and is handed back
 * in calls.  Checked before any launch, TAXOR_E_ARG naming the field: the searcher's `index` is the accumulator's.
 * _add_csr: the same over host arrays (tuples of read r at [read_off[r], read_off[r+1]) of user_bin / count; query_len[n_reads]);
 * a `user_bin` outside the lineage is refused before any launch; calls.n_hashes is NULL; valid until the next _add_csr.
 * _add calls may come from several threads.  Sums are order-free: the tallies do not depend on the order of the calls, on how reads are
 * cut into batches, or on the launch geometry.
 * _results: host pointers, valid until _destroy or the next _results. */
typedef struct taxor_lineage taxor_lineage;
typedef struct {
    uint64_t n_user_bins, n_nodes;
    uint32_t max_depth, reserved;   /* the longest stored path */
    const uint32_t *bin_species;    /* [n_user_bins] */
    const uint64_t *path_off;       /* [n_user_bins + 1] */
    const int32_t *path;            /* [path_off[n_user_bins]] node numbers, root-down */
    const int32_t *parent;          /* [n_nodes] node number or TAXOR_LCA_ROOT */
    const uint32_t *depth;          /* [n_nodes] 1 for ROOT's children */
    const char *const *id;          /* [n_nodes] */
    const char *const *name;        /* [n_nodes] */
    const char *rank;               /* [n_nodes] one letter each, not NUL-terminated */
} taxor_lineage_view;
int taxor_lineage_create(const taxor_hixf_meta *meta, uint64_t n_user_bins, taxor_lineage **out);
int taxor_lineage_get_view(const taxor_lineage *l, taxor_lineage_view *out);
void taxor_lineage_free(taxor_lineage *l);
#define TAXOR_LCA_ROOT (-1)
#define TAXOR_LCA_UNCLASSIFIED (-2)
typedef struct taxor_gpu_lca taxor_gpu_lca;
typedef struct {
    uint64_t n_reads, first_read;
    const int32_t *node;       /* [n_reads] node number, TAXOR_LCA_ROOT or TAXOR_LCA_UNCLASSIFIED */
    const uint32_t *best;      /* [n_reads] the read's maximum count, 0 for an unclassified read */
    const uint32_t *n_refs;    /* [n_reads] surviving tuples, 0 for an unclassified read */
    const uint32_t *n_hashes;  /* [n_reads] QHASH_COUNT (_add_batch), NULL (_add_csr) */
} taxor_lca_calls;
typedef struct {
    uint64_t n_nodes;
    const uint64_t *direct_reads;  /* [n_nodes + 2]: the nodes, then ROOT at n_nodes, UNCLASSIFIED at n_nodes + 1 */
    const uint64_t *direct_bases;  /* [n_nodes + 2] likewise: read lengths summed */
    uint64_t n_reads;              /* reads added so far */
    double seconds_kernel;         /* HIP-event time of the kernel, summed over the calls */
} taxor_lca_results;
int taxor_gpu_lca_create(taxor_gpu_index *idx, const taxor_lineage *lineage, taxor_gpu_lca **out);
int taxor_gpu_lca_add_batch(taxor_gpu_lca *lca, taxor_gpu_searcher *s, uint64_t first_read, taxor_lca_calls *calls);
int taxor_gpu_lca_add_csr(taxor_gpu_lca *lca, uint64_t n_reads, const uint64_t *read_off, const int64_t *user_bin, const uint32_t *count,
                          const uint64_t *query_len, taxor_lca_calls *calls);
int taxor_gpu_lca_results(taxor_gpu_lca *lca, taxor_lca_results *out);
void taxor_gpu_lca_destroy(taxor_gpu_lca *lca);

/* ---- where along a read each reference matched (`taxor search --hitmap-file`; taxor_amd/csrc/hitmap.hip and hitmap_format.h, DESIGN.md
 * section 10.4).  The TSV gives a (read, reference) pair ONE number; a chimeric read, a prophage inside a chromosome read and a read
 * that matches a genome through one conserved operon look alike in it.  The hit map says in which part of the read the hits lie.
 * For read r: n = its saved hash count (the searcher's QHASH_COUNT), T its tuples, m the maximum count over T.  A tuple SURVIVES when
 * !((double)count < (double)m * 0.8), fp64 as written (taxor_classify_filter's expression); a survivor is MAPPED when n > 0 -- a read
 * without a hash reports every leaf with count 0 and the TSV prints those lines, but there is nothing to locate.  Mapped tuples keep the
 * CSR's order, the order of the TSV's lines.
 * Hash i of the read is the i-th entry of its saved list, from 0: the lists are kept in first-insertion order, the order of first
 * occurrence along the read.  It lies in segment seg(i) = floor(i * S / n), 64-bit; segment j holds ceil((j+1) * n / S) - ceil(j * n / S)
 * hashes, none for some j when n < S.  Segments cut the ORDERED HASH LIST, not the bases: a hash list carries no positions.
 * Hash h MATCHES user bin b when the three fingerprints of IXF x at h's rows in column j xor to h's fingerprint -- under the index's
 * arithmetic code and x's seed -- for at least one leaf technical bin (x, j) of b: every bin with fname_idx == b anywhere in the
 * hierarchy, root included (the leaf bins of the coverage accumulator).  hits[t * S + j] = the hashes of segment j that match the user
 * bin of mapped tuple t.  The sum over j may differ from the tuple's count: the search counts per technical bin and adds the parts of a
 * split user bin, a hash found in two parts is one hit here; for a user bin with one leaf technical bin the two are equal.
 * _create: segments S in [1, 64]; `view` is the one the index was created from (only bins and fname_idx are read).  TAXOR_E_ARG naming
 * the reason: segments outside the range; a paged index, by name (its leaf bins are not all resident).
 * _add_batch: after taxor_gpu_search_batch_end (or _batch_sync) of a batch that ran with capture on, with that batch's saved lists
 * (taxor_gpu_search_take_saved, which stay the caller's), before the next batch on the searcher.  Checked before any launch,
 * TAXOR_E_ARG naming the field: the saved batch is sound, its n_reads is the searcher's, its n_hashes are the searcher's, the searcher's
 * index is the hit map's.  The searcher's device-resident CSR is read where it lies; only the lists of reads that have a mapped tuple
 * are staged, through a bounded device buffer.  The result lies in page-locked host memory kept per searcher: valid until the next
 * _add_batch on THAT searcher (or _destroy).  Calls may come from several threads.  hits are integer sums: they do not depend on the
 * launch geometry nor on how reads are cut into pieces, staged groups and batches. */
typedef struct taxor_gpu_hitmap taxor_gpu_hitmap;
typedef struct {
    uint64_t n_reads, n_mapped;
    uint32_t segments, reserved;
    const uint64_t *map_off;       /* [n_reads + 1] read r's mapped tuples are [map_off[r], map_off[r + 1]) of the arrays below */
    const uint64_t *tuple;         /* [n_mapped] the tuple's index in the batch CSR (user_bin / count of taxor_gpu_results) */
    const int64_t *user_bin;       /* [n_mapped] */
    const uint32_t *count;         /* [n_mapped] QHASH_MATCH */
    const uint32_t *hits;          /* [n_mapped * segments] */
    const uint32_t *n_hashes;      /* [n_reads] QHASH_COUNT */
    double seconds_kernels;        /* HIP-event time of this call's kernels */
    uint64_t probes;               /* (hash, leaf bin) lookups made by this call: three one-byte gathers each */
} taxor_hitmap_batch;
int taxor_gpu_hitmap_create(taxor_gpu_index *idx, const taxor_hixf_view *view, uint32_t segments, taxor_gpu_hitmap **out);
int taxor_gpu_hitmap_add_batch(taxor_gpu_hitmap *hm, taxor_gpu_searcher *s, const taxor_gpu_saved *saved, taxor_hitmap_batch *out);
void taxor_gpu_hitmap_destroy(taxor_gpu_hitmap *hm);

/* ---- how much of a read stands behind its LCA call, and the call a threshold on that leaves (`taxor search --lca-confidence`;
 * taxor_amd/csrc/confidence.hip and confidence_format.h).  The call above comes from the survivors of the
 * 0.8 * max filter alone: a read whose best reference holds 12 % of its hashes is called like one that matches at 95 %, and the
 * QHASH_MATCH columns cannot be added up to tell them apart (a hash shared by two references, or found in two parts of a split user
 * bin, counts twice there).
 * For read r: n = its saved hash count (QHASH_COUNT), T = ALL its tuples in the batch CSR, m the maximum count.  The call above stands
 * as defined there: the survivors are the tuples with !((double)count < (double)m * 0.8), P is the longest common prefix of the
 * survivors' compacted paths, D = len(P), the LCA node is P[D-1], ROOT for D = 0.  T empty or m == 0: UNCLASSIFIED, and every word
 * below is 0 for such a read.
 * For a classified read: agree(t), for every tuple t of T, = the length of the common prefix of t's user bin's compacted path and P,
 * in [0, D]; survivors have D.  Hash i (the i-th entry of the read's saved list) MATCHES tuple t when it matches t's user bin by the
 * hit map's lookup above: at least one leaf technical bin of the user bin, under the index's arithmetic code and the IXF's seed.
 * a(i) = the maximum of agree(t) over the tuples hash i matches, undefined if it matches none.  support[d], d = 0..D, = the number of
 * hashes i with a(i) defined and a(i) >= d: a hash counts ONCE, however many references or parts of a split user bin it is found in;
 * support is non-increasing in d; support[0] = the read's hashes found in any reported reference.
 * Given C in [0, 1], depth d HOLDS when !((double)support[d] < C * (double)n), fp64 as written (the object is built with
 * -ffp-contract=off).  The confident call is the deepest d <= D that holds: P[d-1], ROOT for d = 0; if not even d = 0 holds the read
 * is UNCLASSIFIED.  C = 0 gives the call above for every read.  direct_reads / direct_bases are tallied at the confident node.
 * _create: `view` is the one the index was created from (only bins and fname_idx are read).  TAXOR_E_ARG naming the reason: a
 * `confidence` outside [0, 1] or NaN; a paged index, by name; a lineage whose n_user_bins is not the index's.
 * _add_batch: after taxor_gpu_search_batch_end (or _batch_sync) of a batch that ran with capture on, with that batch's saved lists
 * (which stay the caller's), before the next batch on the searcher.  Checked before any launch, TAXOR_E_ARG naming the field: the
 * saved batch is sound, its n_reads is the searcher's, its n_hashes are the searcher's, the searcher's index is the object's.  The
 * searcher's device-resident CSR is read where it lies, the read lengths from the batch's offsets; only the lists of classified reads
 * are staged, through a bounded device buffer.  calls: page-locked host memory kept per searcher, valid until the next _add_batch on
 * THAT searcher (or _destroy).
 * _add_csr: the same over host arrays (tuples of read r at [read_off[r], read_off[r+1]) of user_bin / count; query_len[n_reads]; the
 * read's hash list at [hash_off[r], hash_off[r+1]) of hashes); a `user_bin` outside the lineage is refused before any launch; valid
 * until the next _add_csr.
 * _add calls may come from several threads.  Every word is an integer sum or decided from integer sums: nothing depends on the launch
 * geometry, on the cut into pieces, staged groups and batches, or on the order of the calls.
 * _results: the tallies at the confident nodes, as taxor_gpu_lca_results gives them; seconds_kernel sums this object's kernels. */
typedef struct taxor_gpu_confidence taxor_gpu_confidence;
typedef struct {
    uint64_t n_reads, first_read;
    const int32_t *node;           /* [n_reads] the confident call: node number, TAXOR_LCA_ROOT or TAXOR_LCA_UNCLASSIFIED */
    const uint32_t *depth;         /* [n_reads] its depth d (0 for ROOT and for an unclassified read) */
    const int32_t *lca_node;       /* [n_reads] the call without a threshold */
    const uint32_t *lca_depth;     /* [n_reads] D */
    const uint32_t *support;       /* [n_reads] support[d] at the confident depth; support[0] for a read the threshold made unclassified */
    const uint32_t *lca_support;   /* [n_reads] support[D] */
    const uint32_t *any_support;   /* [n_reads] support[0] */
    const uint32_t *best;          /* [n_reads] the read's maximum count, 0 for a read without an LCA */
    const uint32_t *n_refs;        /* [n_reads] surviving tuples, 0 for a read without an LCA */
    const uint32_t *n_hashes;      /* [n_reads] QHASH_COUNT (_add_csr: the lists' lengths) */
    double seconds_kernels;        /* HIP-event time of this call's kernels */
    uint64_t probes;               /* (hash, leaf bin) lookups made by this call: three one-byte gathers each */
    uint64_t tuple_steps;          /* (64 hashes, tuple) steps that reached the lookup ... */
    uint64_t tuple_steps_full;     /* ... of one per tuple per round of 64 hashes; loop iterations that only read a tuple's agree byte are in neither */
} taxor_confidence_calls;
int taxor_gpu_confidence_create(taxor_gpu_index *idx, const taxor_hixf_view *view, const taxor_lineage *lineage, double confidence,
                                taxor_gpu_confidence **out);
int taxor_gpu_confidence_add_batch(taxor_gpu_confidence *cf, taxor_gpu_searcher *s, const taxor_gpu_saved *saved, uint64_t first_read,
                                   taxor_confidence_calls *calls);
int taxor_gpu_confidence_add_csr(taxor_gpu_confidence *cf, uint64_t n_reads, const uint64_t *read_off, const int64_t *user_bin, const uint32_t *count,
                                 const uint64_t *query_len, const uint64_t *hash_off, const uint64_t *hashes, taxor_confidence_calls *calls);
int taxor_gpu_confidence_results(taxor_gpu_confidence *cf, taxor_lca_results *out);
void taxor_gpu_confidence_destroy(taxor_gpu_confidence *cf);

/* ---- where a read switches reference (`taxor search --breakpoint-file`; taxor_amd/csrc/breakpoint.hip and breakpoint_format.h,
 * DESIGN.md section 10.6).  The hit map above gives one line per reference and sixteen counters; whether a read is a chimera, carries
 * an inserted element or crosses a host/microbe junction needs all of a read's references at once and every position of its list.
 * For read r: n = its saved hash count (QHASH_COUNT); h(0) .. h(n-1) its saved list, in the capture's first-occurrence order; T = ALL
 * its tuples in the batch CSR, not only the survivors of the 0.8 * max filter (the minor partner of a chimera lies below that filter by
 * construction).  The CANDIDATES are the tuples of T with count > 0, in CSR order, numbered c = 0 .. M-1.  The read is EXAMINED when
 * n > 0 and M >= 2; every word below is 0 for a read that is not.
 * x_c(i) = 1 when h(i) matches candidate c's user bin by the hit map's lookup above (at least one leaf technical bin of the user bin,
 * under the index's arithmetic code and the IXF's seed), else 0.  total_c = sum_i x_c(i) (the hit map's LOCATED);
 * pre_c(p) = sum_{i<p} x_c(i); suf_c(p) = total_c - pre_c(p).  For p in [0, n): P(p) = max_c pre_c(p), S(p) = max_c suf_c(p),
 * split(p) = P(p) + S(p).  single = max_c total_c = split(0); best = the lowest c that attains it.  gain = max_p split(p) - single >= 0.
 * The break p* = the smallest p that attains the maximum; A = the lowest c with pre_c(p*) == P(p*), B = the lowest c with
 * suf_c(p*) == S(p*).  Where gain > 0, A != B (A == B gives split(p*) = total_A <= single).  All arithmetic is integer.
 * A read is REPORTED when it is examined and gain >= min_gain.  A partner that did not pass the search threshold is not a tuple and
 * cannot be a candidate: lower the threshold to look for short inserts.
 * _create: `view` is the one the index was created from (only bins and fname_idx are read); min_gain >= 1.  TAXOR_E_ARG naming the
 * reason: min_gain 0; a paged index, by name.
 * _add_batch: after taxor_gpu_search_batch_end (or _batch_sync) of a batch that ran with capture on, with that batch's saved lists
 * (which stay the caller's), before the next batch on the searcher.  Checked before any launch, TAXOR_E_ARG naming the field: the saved
 * batch is sound, its n_reads is the searcher's, its n_hashes are the searcher's, the searcher's index is the object's.  The searcher's
 * device-resident CSR is read where it lies; only the lists of examined reads are staged, through a bounded device buffer.  The match
 * matrix (8 bytes per candidate and 64 hashes, and 4 bytes of prefix counts beside them) lies in device scratch held under a fixed
 * budget per group of reads; a read that exceeds it by itself is processed alone in scratch grown to fit, and an allocation that fails
 * is TAXOR_E_NOMEM naming the bytes: no read is skipped.  The result lies in page-locked host memory kept per searcher: valid until the
 * next _add_batch on THAT searcher (or _destroy).
 * _add_csr: the same over host arrays (tuples of read r at [read_off[r], read_off[r+1]) of user_bin / count; the read's hash list at
 * [hash_off[r], hash_off[r+1]) of hashes); a `user_bin` outside the index is refused before any launch; valid until the next _add_csr.
 * _add calls may come from several threads.  Nothing depends on the launch geometry nor on the cut into pieces, groups and batches. */
typedef struct taxor_gpu_breakpoint taxor_gpu_breakpoint;
typedef struct {
    uint64_t n_reads, n_examined, n_reported;
    uint32_t min_gain, reserved;
    const uint8_t *examined;       /* [n_reads] 1: n > 0 and M >= 2 */
    const uint32_t *gain;          /* [n_reads] */
    const uint32_t *break_hash;    /* [n_reads] p* */
    const uint64_t *tuple_a;       /* [n_reads] index of A in the batch CSR (_add_csr: in user_bin / count as given) */
    const uint64_t *tuple_b;       /* [n_reads] of B */
    const uint64_t *tuple_best;    /* [n_reads] of best */
    const uint32_t *pre_a;         /* [n_reads] pre_A(p*) = P(p*) */
    const uint32_t *suf_b;         /* [n_reads] suf_B(p*) = S(p*) */
    const uint32_t *pre_b;         /* [n_reads] pre_B(p*) */
    const uint32_t *suf_a;         /* [n_reads] suf_A(p*) */
    const uint32_t *single;        /* [n_reads] */
    const uint32_t *n_candidates;  /* [n_reads] M */
    const uint32_t *n;             /* [n_reads] n, 0 for a read that is not examined */
    const uint32_t *n_hashes;      /* [n_reads] QHASH_COUNT of every read (_add_csr: the lists' lengths) */
    const int64_t *bin_a;          /* [n_reads] the user bins of A, B and best, beside the twelve words */
    const int64_t *bin_b;
    const int64_t *bin_best;
    double seconds_kernels;        /* HIP-event time of this call's kernels */
    uint64_t lookups;              /* (hash, leaf bin) lookups made by this call: three one-byte gathers each */
} taxor_breakpoint_batch;
int taxor_gpu_breakpoint_create(taxor_gpu_index *idx, const taxor_hixf_view *view, uint32_t min_gain, taxor_gpu_breakpoint **out);
int taxor_gpu_breakpoint_add_batch(taxor_gpu_breakpoint *bp, taxor_gpu_searcher *s, const taxor_gpu_saved *saved, taxor_breakpoint_batch *out);
int taxor_gpu_breakpoint_add_csr(taxor_gpu_breakpoint *bp, uint64_t n_reads, const uint64_t *read_off, const int64_t *user_bin, const uint32_t *count,
                                 const uint64_t *hash_off, const uint64_t *hashes, taxor_breakpoint_batch *out);
void taxor_gpu_breakpoint_destroy(taxor_gpu_breakpoint *bp);

/* ---- paint a read with its references (`taxor search --segments-file`; taxor_amd/csrc/segments.hip and segments_format.h, DESIGN.md
 * section 10.7).  The breakpoint above is the best SINGLE split between two references; a chromosome read that carries a prophage
 * (A | B | A), a three-way concatemer (A | B | C) and a read across a shared mobile element all come out of it as one break with an
 * unexplained remainder.  This is the optimal segmentation of the read's ordered hash list among ALL its candidates, with a cost per
 * switch: any number of segments, exact integer arithmetic; the single break, the insert and the mosaic are its special cases.
 * For read r take n, h(0) .. h(n-1), the CANDIDATES c = 0 .. M-1 (all tuples of the read with count > 0, in CSR order), x_c(i), `single`
 * and `best` exactly as defined above.  The read is EXAMINED when n > 0 and M >= 2; every word below is 0 for a read that is not.
 * A path is s: [0, n) -> [0, M).  hits(s) = sum_i x_{s(i)}(i); switches(s) = the number of i >= 1 with s(i) != s(i-1);
 * value(s) = (hits(s) - L * switches(s)) * 2^32 - switches(s) in signed 64 bits, L the switch cost, an integer in [1, 2^20].  In words:
 * maximise hits minus L per switch; among the paths that do, take one with the fewest switches -- a switch that gains nothing is never
 * reported.  A read with n >= 2^31 is refused by name: the value would leave 63 bits.
 * The reported path is the one this recurrence builds; its tie rules are part of the definition.
 *   V_c(0) = x_c(0) * 2^32.  For i >= 1: B(i-1) = max_c V_c(i-1); a(i-1) = the lowest c attaining it; J = B(i-1) - (L * 2^32 + 1);
 *   sw_c(i) = (V_c(i-1) < J), so a tie stays; V_c(i) = x_c(i) * 2^32 + max(V_c(i-1), J).
 *   End: e = a(n-1), value = B(n-1).  Backtrace: s(n-1) = e; for i = n-1 .. 1: s(i-1) = sw_{s(i)}(i) ? a(i-1) : s(i).
 * Consequences: V never decreases and is never negative; sw_{a(i-1)}(i) is never set, so every switch changes the candidate;
 * hits - L * switches >= single (the path that stays on `best` has value single * 2^32).
 * Segments are the maximal runs of s; K = switches + 1.  Segment j carries [start_j, end_j), its candidate c_j,
 * hits_j = sum_{i in segment} x_{c_j}(i) and best_hits_j, the same sum for `best`.  A read is REPORTED when it is examined and K >= 2.
 * The SHAPE of a reported read (segments_format.h, on the host, from the user bins of its segments alone): `split` when K == 2,
 * `insert` when K == 3 and segments 0 and 2 have the same user bin, `mosaic` otherwise.
 * _create: `view` is the one the index was created from (only bins and fname_idx are read).  TAXOR_E_ARG naming the reason: a
 * switch_cost of 0 or above 2^20; a paged index, by name.
 * _add_batch: as taxor_gpu_breakpoint_add_batch, with its checks before any launch.  Scratch per examined read: 8 * M * ceil(n / 64)
 * bytes of match masks, as many of switch words, 4 * 64 * ceil(n / 64) of a, 8 * M of state; groups of reads are held under a fixed
 * budget of 2^23 mask words; a read that exceeds it by itself runs alone in scratch grown to fit, and an allocation that fails is
 * TAXOR_E_NOMEM naming the bytes and the read: no read is skipped.  The result lies in page-locked host memory kept per searcher: valid
 * until the next _add_batch on THAT searcher (or _destroy).
 * _add_csr: the same over host arrays, as taxor_gpu_breakpoint_add_csr; a `user_bin` outside the index is refused before any launch;
 * the same user bin may stand in several tuples; valid until the next _add_csr.
 * _add calls may come from several threads.  Nothing depends on the launch geometry nor on the cut into pieces, groups and batches. */
typedef struct taxor_gpu_segments taxor_gpu_segments;
typedef struct {
    uint64_t n_reads, n_examined, n_reported;
    uint32_t switch_cost;
    uint32_t n_groups;              /* groups of reads the scratch budget cut the examined reads into (0 when none is examined); never moves a result */
    const uint8_t *examined;        /* [n_reads] 1: n > 0 and M >= 2 */
    const uint32_t *n_candidates;   /* [n_reads] M */
    const uint32_t *n;              /* [n_reads] n, 0 for a read that is not examined */
    const uint32_t *n_hashes;       /* [n_reads] QHASH_COUNT of every read (_add_csr: the lists' lengths) */
    const uint32_t *n_segments;     /* [n_reads] K: 0 when not examined, 1 when examined and unbroken */
    const uint32_t *path_hits;      /* [n_reads] hits(s) of the reported path */
    const uint32_t *path_switches;  /* [n_reads] K - 1 */
    const uint32_t *single;         /* [n_reads] */
    const uint64_t *tuple_best;     /* [n_reads] index of best in the batch CSR (_add_csr: in user_bin / count as given) */
    const int64_t *bin_best;        /* [n_reads] its user bin */
    const uint64_t *seg_off;        /* [n_reads + 1] a reported read's K segments are [seg_off[r], seg_off[r + 1]); none otherwise */
    const uint32_t *seg_start;      /* per segment, in list order (null when no read is reported): [start, end) in the hash list */
    const uint32_t *seg_end;
    const uint64_t *seg_tuple;      /* index of the segment's candidate in the batch CSR */
    const int64_t *seg_bin;         /* its user bin */
    const uint32_t *seg_hits;       /* hits_j; their sum over a read is path_hits */
    const uint32_t *seg_best_hits;  /* best_hits_j */
    double seconds_kernels;         /* HIP-event time of this call's kernels */
    uint64_t lookups;               /* (hash, leaf bin) lookups made by this call: three one-byte gathers each */
} taxor_segments_batch;
int taxor_gpu_segments_create(taxor_gpu_index *idx, const taxor_hixf_view *view, uint32_t switch_cost, taxor_gpu_segments **out);
int taxor_gpu_segments_add_batch(taxor_gpu_segments *sg, taxor_gpu_searcher *s, const taxor_gpu_saved *saved, taxor_segments_batch *out);
int taxor_gpu_segments_add_csr(taxor_gpu_segments *sg, uint64_t n_reads, const uint64_t *read_off, const int64_t *user_bin, const uint32_t *count,
                               const uint64_t *hash_off, const uint64_t *hashes, taxor_segments_batch *out);
void taxor_gpu_segments_destroy(taxor_gpu_segments *sg);

/* ---- hashes only one reference explains (`taxor search --exclusive-file` / `--exclusive-reads-file`; taxor_amd/csrc/exclusive.hip and
 * exclusive_format.h).  Near-identical references all pass the 0.8 * max filter with almost the same count; the
 * coverage table counts a shared hash for each of them and the LCA confidence counts it once for none.  This says which of the
 * references a read reported holds hashes that none of the others on that read's list holds, and how many.
 * For read r take n, h(0) .. h(n-1), T (ALL its tuples in the batch CSR), the CANDIDATES c = 0 .. M-1 (the tuples of T with count > 0, in
 * CSR order) and x_c(i) exactly as defined for the breakpoint above.  The read is EXAMINED when n > 0 and M >= 1 -- one candidate is
 * enough here; every word below is 0 for a read that is not.  All arithmetic is integer.
 *   k(i) = sum_c x_c(i).  Hash i is EXCLUSIVE TO c when x_c(i) == 1 and k(i) == 1, SHARED when k(i) >= 2, UNMATCHED when k(i) == 0.
 *   Per candidate: hits_c = sum_i x_c(i) -- the hit map's located hashes, which for a split user bin may differ from the tuple's count,
 *   as said there; excl_c = #{i : i exclusive to c}.  Per read: shared = #{i : k(i) >= 2}, matched = #{i : k(i) >= 1}.
 *   Hence sum_c excl_c + shared == matched <= n; excl_c <= hits_c; sum_c hits_c >= matched; M == 1 gives excl_0 == hits_0.
 * A user bin that stands in two tuples of one read is possible only in hand-made input (_add_csr): both candidates then match the same
 * hashes, so neither has an exclusive one.  That follows from the definition and is not treated specially.
 * Per user bin b, summed over every examined read and every candidate c of it whose user bin is b, in 64 bits on the device:
 *   cand_reads[b] += 1, hits[b] += hits_c, exclusive_hits[b] += excl_c, exclusive_reads[b] += (excl_c > 0);
 * and every hash exclusive to c goes into b's HyperLogLog sketch: (i, rho) = taxor_hll_slot(h, P), registers[b][i] = max(registers[b][i], rho)
 * -- the coverage accumulator's slot, byte registers and estimator (taxor_hll_estimate).
 * Exclusivity is relative to the references the read REPORTED: a reference below the search threshold is not a tuple and takes no hash
 * away.  And fingerprints have 8 bits: a foreign leaf bin answers yes at about 1/256, so a truly exclusive hash is lost at about (leaf
 * bins of the other candidates) / 256 and a candidate that shares nothing still shows about n * leaves / 256 hits, most of them exclusive.
 * _create: precision P in [4, 16], 0 = 12; `view` is the one the index was created from (only bins and fname_idx are read).  The
 * registers (n_user_bins << P bytes) and the counters are held against the device's free memory first: TAXOR_E_NOMEM with both
 * figures.  A paged index is refused by name (TAXOR_E_ARG).
 * _add_batch: as taxor_gpu_breakpoint_add_batch, with its checks before any launch, TAXOR_E_ARG naming the field.  Scratch per examined
 * read is 8 * M bytes (hits and excl, which are the result) beside two words per read of the batch; there is no per-hash array, so
 * reads are not grouped under a budget and none is skipped.  Only the lists of examined reads are staged, through a bounded device
 * buffer.  The batch lies in page-locked host memory kept per searcher: valid until the next _add_batch on THAT searcher (or _destroy).
 * _add_csr: the same over host arrays, as taxor_gpu_breakpoint_add_csr; a `user_bin` outside the index is refused before any launch;
 * valid until the next _add_csr.
 * _results: the run's sums and registers; host pointers, valid until _destroy or the next _results.
 * _add calls may come from several threads.  Sums are integer additions and registers a maximum: nothing depends on the launch geometry,
 * the order of the calls nor on the cut into pieces and batches. */
typedef struct taxor_gpu_exclusive taxor_gpu_exclusive;
typedef struct {
    uint64_t n_reads, n_examined, n_cand;   /* n_cand = cand_off[n_reads]: the candidates of the examined reads */
    uint32_t precision, reserved;
    const uint8_t *examined;        /* [n_reads] 1: n > 0 and M >= 1 */
    const uint32_t *n_candidates;   /* [n_reads] M */
    const uint32_t *n;              /* [n_reads] n, 0 for a read that is not examined */
    const uint32_t *matched;        /* [n_reads] */
    const uint32_t *shared;         /* [n_reads] */
    const uint32_t *n_hashes;       /* [n_reads] QHASH_COUNT of every read (_add_csr: the lists' lengths) */
    const uint64_t *cand_off;       /* [n_reads + 1] an examined read's M candidates are [cand_off[r], cand_off[r + 1]); none otherwise */
    const uint64_t *cand_tuple;     /* per candidate, in CSR order (null when no read is examined): index in the batch CSR (_add_csr: in
                                       user_bin / count as given) */
    const int64_t *cand_bin;        /* its user bin */
    const uint32_t *cand_count;     /* the tuple's count (QHASH_MATCH) */
    const uint32_t *cand_hits;      /* hits_c */
    const uint32_t *cand_excl;      /* excl_c */
    double seconds_kernels;         /* HIP-event time of this call's kernels */
    uint64_t probes;                /* (hash, leaf bin) lookups made by this call: three one-byte gathers each */
} taxor_exclusive_batch;
typedef struct {
    uint64_t n_user_bins;
    uint32_t precision, reserved;
    const uint64_t *cand_reads;       /* [n_user_bins] */
    const uint64_t *hits;             /* [n_user_bins] */
    const uint64_t *exclusive_hits;   /* [n_user_bins] */
    const uint64_t *exclusive_reads;  /* [n_user_bins] */
    const uint8_t *registers;         /* [n_user_bins << precision] user bin b's sketch at registers + (b << precision) */
    double seconds_kernels;           /* summed over the calls */
    uint64_t probes;
} taxor_exclusive_results;
int taxor_gpu_exclusive_create(taxor_gpu_index *idx, const taxor_hixf_view *view, uint32_t precision, taxor_gpu_exclusive **out);
int taxor_gpu_exclusive_add_batch(taxor_gpu_exclusive *ex, taxor_gpu_searcher *s, const taxor_gpu_saved *saved, taxor_exclusive_batch *out);
int taxor_gpu_exclusive_add_csr(taxor_gpu_exclusive *ex, uint64_t n_reads, const uint64_t *read_off, const int64_t *user_bin, const uint32_t *count,
                                const uint64_t *hash_off, const uint64_t *hashes, taxor_exclusive_batch *out);
int taxor_gpu_exclusive_results(taxor_gpu_exclusive *ex, taxor_exclusive_results *out);
void taxor_gpu_exclusive_destroy(taxor_gpu_exclusive *ex);

/* ---- index hashes per reference, read off the resident filter (`taxor census`, `taxor search --coverage-breadth`;
 * taxor_amd/csrc/census.hip and census_format.h).  For every IXF x of the index and every bin j < bins,
 * nonzero[bin_first[x] + j] = #{rows r < 3 * seg_len : data[r * stride + j] != 0}, an exact integer; padding columns bins <= j < stride
 * are not reported and reach no reported bin.  A bin of an interleaved XOR filter gives each of its n keys one slot of its column and
 * leaves the others at the 0 the builder cleared them to, and an assigned slot is uniform over 256 values: nonzero ~ Binomial(n, 255/256),
 * nonzero <= n, and taxor_census_keys_est(nonzero) = llround(nonzero * 256 / 255) estimates n with standard deviation sqrt(n / 255).  A
 * column with more nonzero bytes than taxor_census_capacity(seg_len) is no peeled filter (taxor_gpu_index_fill_random, a writer that
 * does not clear free slots): its estimate says nothing.
 * _create: the work list is cut from the index's descriptors in the search layout (an index loaded under another ixf_layout was
 * transposed into it).  A paged index is refused by name (TAXOR_E_ARG): its IXFs are not all resident.
 * _run: one streaming pass over the fingerprints -- every byte is read once; the counters are zeroed per call, so two calls give the same
 * words.  tile_iters (rows per thread and tile) and max_blocks (the grid) are for tests and A/B runs, 0 = the defaults: the words do not
 * depend on either.  Host pointers, valid until the next _run or _destroy; one _run at a time per object. */
typedef struct taxor_gpu_census taxor_gpu_census;
typedef struct {
    uint64_t n_ixf, n_bins, n_user_bins;   /* n_bins = bin_first[n_ixf]: the technical bins of all IXFs */
    const uint64_t *bin_first;             /* [n_ixf + 1] */
    const uint64_t *nonzero;               /* [n_bins] in index bin order: all bins of IXF 0, then IXF 1, ... */
    double seconds_kernel;                 /* HIP-event time of the launches */
    uint64_t bytes_read;                   /* fingerprint bytes of the index, padding columns included: each read once */
    uint64_t n_tiles;                      /* work items */
    uint32_t launches, reserved;
} taxor_census_results;
int taxor_gpu_census_create(taxor_gpu_index *idx, taxor_gpu_census **out);
int taxor_gpu_census_run(taxor_gpu_census *c, uint32_t tile_iters, uint32_t max_blocks, taxor_census_results *out);
void taxor_gpu_census_destroy(taxor_gpu_census *c);
/* Host only: census_format.h for a binding.  _peeled: nonzero <= capacity(seg_len).  The _line functions write the text of one line of
 * `taxor census`'s two files (flagged != 0: the count is NA), _breadth_columns the four columns `--coverage-breadth` appends, into buf
 * (NUL-terminated, truncated to cap) and return the full length */
uint64_t taxor_census_keys_est(uint64_t nonzero);
uint64_t taxor_census_capacity(uint64_t seg_len);
int taxor_census_peeled(uint64_t nonzero, uint64_t seg_len);
uint64_t taxor_census_ref_line(const char *accession, const char *name, const char *taxid, uint64_t ref_len, uint64_t leaf_bins, uint64_t index_hashes, int flagged,
                               char *buf, uint64_t cap);
uint64_t taxor_census_ixf_line(uint64_t ixf, uint64_t bins, uint64_t leaf_bins, uint64_t seg_len, uint64_t stride, uint64_t max_bin_keys, int flagged, char *buf,
                               uint64_t cap);
uint64_t taxor_census_breadth_columns(uint64_t distinct, uint64_t hash_matches, uint64_t index_hashes, int flagged, char *buf, uint64_t cap);

/* ---- search straight from file bytes (taxor_amd/csrc/fastx_scan.hip): raw[0, n_bytes) holds whole records of one
 * kind, '>' (FASTA) or '@' (four-line FASTQ) -- what a reader cuts at record boundaries.  The device finds the records, packs their
 * sequences into the searcher's batch and runs the search; taxor_gpu_search_batch_end follows as after any _begin.  raw may be pageable
 * or registered with taxor_gpu_host_register, and is free again when the call returns.  The table's pointers stay valid until the next
 * call on the searcher.  An id is the header line without its first character and without the line terminator.
 * status TAXOR_FASTX_IRREGULAR (the call returns TAXOR_OK): the bytes are not plain records of that kind -- a blank line between FASTQ
 * records, a wrapped FASTQ sequence, a quality line of another length, a first non-blank byte that is not the record character.  Nothing
 * was enqueued and the table is empty: parse the bytes on the host.  A byte outside dna15 in a sequence is TAXOR_E_ALPHABET.  The reads go
 * through the batch pipeline as one resident batch (sub_batch_reads / sub_batch_bases and the threshold models apply as for any batch; the
 * lanes for small calls are not used: the bytes are on the device already).  n_bytes >= 2^40 is TAXOR_E_ARG. */
#define TAXOR_FASTX_IRREGULAR 1u
typedef struct {
    uint64_t n_reads;
    const uint64_t *id_off, *id_len;   /* [n_reads], byte positions inside raw */
    const uint64_t *read_len;          /* [n_reads] */
    uint32_t status;                   /* 0, or TAXOR_FASTX_IRREGULAR: nothing was enqueued, parse on the host */
} taxor_fastx_scan;
int taxor_gpu_search_fastx_begin(taxor_gpu_searcher *s, const char *raw, uint64_t n_bytes, int kind, taxor_fastx_scan *scan);

/* ---- search from 4-bit sequences (taxor_amd/csrc/bam_pack.hip): what a BAM record's SEQ field holds, two bases per
 * byte, the first in the high nibble, codes of the alphabet "=ACMGRSVTWYHKDBN".  Read i of a segment is read_len[i] bases from byte
 * byte_off[i] of seq4 (every read starts on a byte; the low nibble of an odd read's last byte is ignored); reverse[i] != 0 says that the
 * read is stored reverse-complemented and is restored on the device -- the complement is taken on the IUPAC code before the dna4
 * mapping.  reverse == NULL: every read is forward.  The reads of all segments form ONE resident batch in segment order, like
 * taxor_gpu_search_fastx_begin's (sub_batch_reads / sub_batch_bases, the processing order and the threshold models apply as for any
 * batch; the lanes for small calls are not used); taxor_gpu_search_batch_end follows.  The arrays are free again when the call returns.
 * Checked before anything is launched (TAXOR_E_ARG): null pointers, byte offsets that do not ascend or lie inside the read before,
 * read_len >= 2^31, a segment of 2^40 bytes or more.  Nibble 0 ('=') is not dna15: TAXOR_E_ALPHABET.  Works on a searcher of a paged
 * index (taxor_gpu_results_keys, taxor_gpu_search_merge_prior).  The segment type stands with taxor_gpu_pack_nibbles above. */
int taxor_gpu_search_nibbles_begin(taxor_gpu_searcher *s, const taxor_nibble_segment *segs, uint64_t n_segs);

#ifdef __cplusplus
}
#endif
#endif
