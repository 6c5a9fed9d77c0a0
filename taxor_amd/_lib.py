"""ctypes binding of libtaxor_gpu.so (include/taxor_gpu.h).  There is no fallback: if the HIP library is
missing or does not load, importing anything that computes raises immediately."""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "libtaxor_gpu.so")
CSRC = os.path.join(_HERE, "csrc")


def build(force=False):
    """Compile the HIP library in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    args = ["make", "-C", CSRC, "-s"] + (["-B"] if force else [])
    subprocess.check_call(args)
    return SO_PATH


class IxfView(C.Structure):
    _fields_ = [("bins", C.c_uint64), ("stride", C.c_uint64), ("seg_len", C.c_uint64), ("seed", C.c_uint64),
                ("data", C.c_void_p), ("next_ixf", C.c_void_p), ("fname_idx", C.c_void_p), ("src_stride", C.c_uint64)]


IXF_READ_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p)


class IxfSource(C.Structure):
    _fields_ = [("read", IXF_READ_FN), ("ctx", C.c_void_p)]


class HixfView(C.Structure):
    _fields_ = [("n_ixf", C.c_uint64), ("ixf", C.POINTER(IxfView)), ("n_user_bins", C.c_uint64),
                ("kmer_size", C.c_uint8), ("syncmer_size", C.c_uint8), ("t_syncmer", C.c_uint8),
                ("use_syncmer", C.c_uint8), ("scaling", C.c_uint16), ("window_size", C.c_uint64), ("ixf_arith", C.c_uint32),
                ("source", C.c_void_p), ("ixf_layout", C.c_uint32)]


class ReadSegment(C.Structure):
    _fields_ = [("bases", C.c_void_p), ("offsets", C.c_void_p), ("n_reads", C.c_uint64)]


class SearchParams(C.Structure):
    _fields_ = [("ratio", C.c_double), ("sub_batch_reads", C.c_uint32), ("sub_batch_bases", C.c_uint64),
                ("time_kernels", C.c_uint32), ("model", C.c_uint32), ("error_rate", C.c_double), ("flags", C.c_uint32)]


SEARCH_NO_PRUNE, SEARCH_GROUP_ALWAYS, SEARCH_NO_SMALL_PATH, SEARCH_SPLIT_ALWAYS, SEARCH_FORCE_TREE_STALL = 1, 2, 4, 8, 16
SEARCH_NO_SCREEN = 32


THR_PERCENTAGE, THR_SYNCMER, THR_KMER, THR_FRACMINHASH = 0, 1, 2, 3


class Results(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_tuples", C.c_uint64), ("read_off", C.POINTER(C.c_uint64)),
                ("user_bin", C.POINTER(C.c_int64)), ("count", C.POINTER(C.c_uint32)),
                ("n_hashes", C.POINTER(C.c_uint32))]


class RunStats(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_bases", C.c_uint64), ("n_hashes", C.c_uint64),
                ("n_tuples", C.c_uint64), ("n_work_items", C.c_uint64), ("algorithmic_bytes", C.c_uint64),
                ("query_bytes", C.c_uint64), ("query_touched_bytes", C.c_uint64), ("query_launches", C.c_uint32), ("query_ms", C.c_float),
                ("syncmer_ms", C.c_float), ("finalize_ms", C.c_float), ("total_ms", C.c_float),
                ("level_ms", C.c_float * 8), ("level_requested_bytes", C.c_uint64 * 8), ("level_row_reads", C.c_uint64 * 8),
                ("level_sparse_loads", C.c_uint64 * 8), ("tree_stalls_recovered", C.c_uint32), ("small_pieces_rerun", C.c_uint32),
                ("screen_plane_loads", C.c_uint64)]


class CommStats(C.Structure):
    _fields_ = [("transport", C.c_int32), ("n_devices", C.c_uint32), ("index_bytes", C.c_uint64), ("index_upload_bytes", C.c_uint64),
                ("index_broadcast_bytes", C.c_uint64), ("index_seconds", C.c_double), ("gathers", C.c_uint64),
                ("gather_bytes", C.c_uint64), ("gather_seconds", C.c_double), ("index_broadcast_calls", C.c_uint64),
                ("self_exchange_bytes", C.c_uint64), ("rccl_version", C.c_int32), ("selftest_bytes", C.c_uint64)]


COMM_RCCL, COMM_HOST = 0, 1


class Species(C.Structure):
    _fields_ = [("organism_name", C.c_char_p), ("accession_id", C.c_char_p), ("taxid", C.c_char_p),
                ("taxnames_string", C.c_char_p), ("taxid_string", C.c_char_p), ("user_bin", C.c_uint64),
                ("seq_len", C.c_uint64)]


class HixfMeta(C.Structure):
    _fields_ = [("window_size", C.c_uint64), ("parts", C.c_uint8), ("compressed", C.c_uint8),
                ("n_species", C.c_uint64), ("species", C.POINTER(Species)), ("n_user_bin_filenames", C.c_uint64),
                ("user_bin_filenames", C.POINTER(C.c_char_p)), ("foreign_schema", C.c_uint8)]


class IxfSchema(C.Structure):
    _fields_ = [("n_before", C.c_uint32), ("n_after", C.c_uint32), ("idx_bins", C.c_int32), ("idx_stride", C.c_int32),
                ("idx_seg_len", C.c_int32), ("idx_seed", C.c_int32), ("seg_len_is_rows", C.c_uint32),
                ("default_seed", C.c_uint64), ("layout", C.c_uint32), ("len_unit", C.c_uint32), ("skip_before_len", C.c_uint32),
                ("skip_after_len", C.c_uint32)]


class IxfVariant(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("seg_len", C.c_uint64), ("stride", C.c_uint64), ("key_hash", C.c_uint8),
                ("seed_mode", C.c_uint8), ("rot", C.c_uint8), ("reduce", C.c_uint8), ("fp_mode", C.c_uint8),
                ("pad", C.c_uint8), ("layout", C.c_uint16)]


# layout codes (taxor_amd/csrc/ixf_layout.h)
LAYOUT_ROWS, LAYOUT_BIN_MAJOR, LAYOUT_BIT_SLICED = 0, 1, 2
LAYOUT_POSITION_MAJOR, LAYOUT_PITCH_BINS, LAYOUT_PITCH_STORED = 0x100, 0x200, 0x400

# every symbol include/taxor_gpu.h and include/taxor_gpu_tools.h declare: name -> (restype, argtypes)
_P = C.c_void_p
class BuildStats(C.Structure):
    _fields_ = [("keys_inserted", C.c_uint64), ("scratch_bytes", C.c_uint64), ("rounds_max", C.c_uint32), ("reseeds", C.c_uint32),
                ("chunks", C.c_uint32), ("reserved", C.c_uint32), ("seconds_peel", C.c_double), ("seconds_assign", C.c_double),
                ("seconds_union", C.c_double), ("seconds_total", C.c_double), ("seconds_release", C.c_double),
                ("seconds_count", C.c_double), ("seconds_rounds", C.c_double), ("seconds_upload", C.c_double),
                ("seconds_alloc", C.c_double), ("keys_counted_in_lds", C.c_uint64),
                ("stream_groups", C.c_uint32), ("stream_ranges", C.c_uint32), ("stream_restarts", C.c_uint32), ("reserved2", C.c_uint32),
                ("stream_bytes_uploaded", C.c_uint64), ("seconds_stream_upload", C.c_double), ("seconds_stream_upload_wait", C.c_double)]


class KeyerParams(C.Structure):
    _fields_ = [("kmer_size", C.c_uint32), ("syncmer_size", C.c_uint32), ("t_syncmer", C.c_uint32), ("use_syncmer", C.c_uint32),
                ("window_size", C.c_uint64), ("scaling", C.c_uint32), ("reserved", C.c_uint32), ("n_bins", C.c_uint64)]


class KeyerStats(C.Structure):
    _fields_ = [("calls", C.c_uint64), ("records", C.c_uint64), ("bases", C.c_uint64), ("tiles", C.c_uint64), ("call_keys", C.c_uint64),
                ("keys", C.c_uint64), ("seconds_device", C.c_double), ("seconds_add", C.c_double), ("seconds_finish", C.c_double)]


class Layout(C.Structure):
    _fields_ = [("n_ixf", C.c_uint64), ("n_bins_total", C.c_uint64), ("t_max", C.c_uint64), ("depth", C.c_uint32), ("reserved", C.c_uint32),
                ("bytes_per_hash", C.c_double), ("index_bytes", C.c_double), ("ixf_bins", C.POINTER(C.c_uint64)),
                ("bin_first", C.POINTER(C.c_uint64)), ("next_ixf", C.POINTER(C.c_int64)), ("fname_idx", C.POINTER(C.c_int64)),
                ("part", C.POINTER(C.c_uint64)), ("parts", C.POINTER(C.c_uint64))]


class ProfileCsr(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_refs", C.c_uint64), ("n_matches", C.c_uint64), ("read_off", C.c_void_p), ("ref", C.c_void_p),
                ("ref_len", C.c_void_p), ("hash_match", C.c_void_p), ("query_len", C.c_void_p), ("hash_count", C.c_void_p)]


class ProfileResults(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_refs", C.c_uint64), ("n_matches", C.c_uint64), ("ref", C.POINTER(C.c_int32)),
                ("ref_len", C.POINTER(C.c_uint64)), ("alive", C.POINTER(C.c_uint8)), ("best", C.POINTER(C.c_uint8)),
                ("has_prior", C.POINTER(C.c_uint8)), ("taxa_len", C.POINTER(C.c_uint64)), ("ref_nts", C.POINTER(C.c_uint64)),
                ("log_prior", C.POINTER(C.c_double)), ("explained_by", C.POINTER(C.c_int32)), ("unique_reads", C.POINTER(C.c_uint32)),
                ("all_reads", C.POINTER(C.c_uint32)), ("all_nts", C.c_uint64), ("unclassified_nts", C.c_uint64),
                ("log_unclassified", C.c_double), ("em_steps_needed", C.c_uint32), ("em_iterations", C.c_uint32), ("n_pairs", C.c_uint64),
                ("pair_slots", C.c_uint64), ("pair_key", C.POINTER(C.c_uint64)), ("pair_count", C.POINTER(C.c_uint32)),
                ("alive_round1", C.POINTER(C.c_uint8)), ("alive_round2", C.POINTER(C.c_uint8)), ("alive_round3", C.POINTER(C.c_uint8)),
                ("iter_ref_nts", C.POINTER(C.c_uint64)), ("seconds_filter", C.c_double), ("seconds_em", C.c_double)]


BINS_CLEAR, BINS_CLEARED = 1, 2
PROFILE_TRACE = 1
FEED_KEEP_ALL = 1


class FastxScan(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("id_off", C.POINTER(C.c_uint64)), ("id_len", C.POINTER(C.c_uint64)),
                ("read_len", C.POINTER(C.c_uint64)), ("status", C.c_uint32)]


FASTX_IRREGULAR = 1


class NibbleSegment(C.Structure):
    _fields_ = [("seq4", C.c_void_p), ("byte_off", C.c_void_p), ("read_len", C.c_void_p), ("reverse", C.c_void_p), ("n_reads", C.c_uint64)]


class PassPlan(C.Structure):
    _fields_ = [("n_passes", C.c_uint32), ("n_subtrees", C.c_uint32), ("root_bytes", C.c_uint64), ("slab_bytes", C.c_uint64),
                ("index_bytes", C.c_uint64)]


class Prior(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_tuples", C.c_uint64), ("read_off", C.c_void_p), ("user_bin", C.c_void_p),
                ("count", C.c_void_p), ("key", C.c_void_p)]


PASS_ROOT = 0xFFFFFFFF


class SavedView(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("total_hashes", C.c_uint64), ("n_sub_batches", C.c_uint64), ("read_len", C.POINTER(C.c_uint32)),
                ("n_hashes", C.POINTER(C.c_uint32)), ("threshold", C.POINTER(C.c_uint64)), ("hash_off", C.POINTER(C.c_uint64)),
                ("hashes", C.POINTER(C.c_uint64)), ("sub_first", C.POINTER(C.c_uint32)), ("order", C.POINTER(C.c_uint32)),
                ("use_syncmer", C.c_uint32), ("kmer_size", C.c_uint32), ("syncmer_size", C.c_uint32), ("t_syncmer", C.c_uint32),
                ("scaling", C.c_uint32), ("model", C.c_uint32), ("window_size", C.c_uint64), ("error_rate", C.c_double), ("ratio", C.c_double)]


class CoverageResults(C.Structure):
    _fields_ = [("n_user_bins", C.c_uint64), ("precision", C.c_uint32), ("reserved", C.c_uint32), ("reads", C.POINTER(C.c_uint64)),
                ("hash_matches", C.POINTER(C.c_uint64)), ("registers", C.POINTER(C.c_uint8)), ("seconds_kernels", C.c_double),
                ("probes", C.c_uint64)]


class LineageView(C.Structure):
    _fields_ = [("n_user_bins", C.c_uint64), ("n_nodes", C.c_uint64), ("max_depth", C.c_uint32), ("reserved", C.c_uint32),
                ("bin_species", C.POINTER(C.c_uint32)), ("path_off", C.POINTER(C.c_uint64)), ("path", C.POINTER(C.c_int32)),
                ("parent", C.POINTER(C.c_int32)), ("depth", C.POINTER(C.c_uint32)), ("id", C.POINTER(C.c_char_p)),
                ("name", C.POINTER(C.c_char_p)), ("rank", C.POINTER(C.c_char))]


LCA_ROOT, LCA_UNCLASSIFIED = -1, -2


class LcaCalls(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("first_read", C.c_uint64), ("node", C.POINTER(C.c_int32)), ("best", C.POINTER(C.c_uint32)),
                ("n_refs", C.POINTER(C.c_uint32)), ("n_hashes", C.POINTER(C.c_uint32))]


class LcaResults(C.Structure):
    _fields_ = [("n_nodes", C.c_uint64), ("direct_reads", C.POINTER(C.c_uint64)), ("direct_bases", C.POINTER(C.c_uint64)),
                ("n_reads", C.c_uint64), ("seconds_kernel", C.c_double)]


class ConfidenceCalls(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("first_read", C.c_uint64), ("node", C.POINTER(C.c_int32)), ("depth", C.POINTER(C.c_uint32)),
                ("lca_node", C.POINTER(C.c_int32)), ("lca_depth", C.POINTER(C.c_uint32)), ("support", C.POINTER(C.c_uint32)),
                ("lca_support", C.POINTER(C.c_uint32)), ("any_support", C.POINTER(C.c_uint32)), ("best", C.POINTER(C.c_uint32)),
                ("n_refs", C.POINTER(C.c_uint32)), ("n_hashes", C.POINTER(C.c_uint32)), ("seconds_kernels", C.c_double), ("probes", C.c_uint64),
                ("tuple_steps", C.c_uint64), ("tuple_steps_full", C.c_uint64)]


class BreakpointBatch(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_examined", C.c_uint64), ("n_reported", C.c_uint64), ("min_gain", C.c_uint32), ("reserved", C.c_uint32),
                ("examined", C.POINTER(C.c_uint8)), ("gain", C.POINTER(C.c_uint32)), ("break_hash", C.POINTER(C.c_uint32)),
                ("tuple_a", C.POINTER(C.c_uint64)), ("tuple_b", C.POINTER(C.c_uint64)), ("tuple_best", C.POINTER(C.c_uint64)),
                ("pre_a", C.POINTER(C.c_uint32)), ("suf_b", C.POINTER(C.c_uint32)), ("pre_b", C.POINTER(C.c_uint32)), ("suf_a", C.POINTER(C.c_uint32)),
                ("single", C.POINTER(C.c_uint32)), ("n_candidates", C.POINTER(C.c_uint32)), ("n", C.POINTER(C.c_uint32)), ("n_hashes", C.POINTER(C.c_uint32)),
                ("bin_a", C.POINTER(C.c_int64)), ("bin_b", C.POINTER(C.c_int64)), ("bin_best", C.POINTER(C.c_int64)),
                ("seconds_kernels", C.c_double), ("lookups", C.c_uint64)]


class SegmentsBatch(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_examined", C.c_uint64), ("n_reported", C.c_uint64), ("switch_cost", C.c_uint32), ("n_groups", C.c_uint32),
                ("examined", C.POINTER(C.c_uint8)), ("n_candidates", C.POINTER(C.c_uint32)), ("n", C.POINTER(C.c_uint32)), ("n_hashes", C.POINTER(C.c_uint32)),
                ("n_segments", C.POINTER(C.c_uint32)), ("path_hits", C.POINTER(C.c_uint32)), ("path_switches", C.POINTER(C.c_uint32)),
                ("single", C.POINTER(C.c_uint32)), ("tuple_best", C.POINTER(C.c_uint64)), ("bin_best", C.POINTER(C.c_int64)),
                ("seg_off", C.POINTER(C.c_uint64)), ("seg_start", C.POINTER(C.c_uint32)), ("seg_end", C.POINTER(C.c_uint32)),
                ("seg_tuple", C.POINTER(C.c_uint64)), ("seg_bin", C.POINTER(C.c_int64)), ("seg_hits", C.POINTER(C.c_uint32)),
                ("seg_best_hits", C.POINTER(C.c_uint32)), ("seconds_kernels", C.c_double), ("lookups", C.c_uint64)]


class ExclusiveBatch(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_examined", C.c_uint64), ("n_cand", C.c_uint64), ("precision", C.c_uint32), ("reserved", C.c_uint32),
                ("examined", C.POINTER(C.c_uint8)), ("n_candidates", C.POINTER(C.c_uint32)), ("n", C.POINTER(C.c_uint32)), ("matched", C.POINTER(C.c_uint32)),
                ("shared", C.POINTER(C.c_uint32)), ("n_hashes", C.POINTER(C.c_uint32)), ("cand_off", C.POINTER(C.c_uint64)),
                ("cand_tuple", C.POINTER(C.c_uint64)), ("cand_bin", C.POINTER(C.c_int64)), ("cand_count", C.POINTER(C.c_uint32)),
                ("cand_hits", C.POINTER(C.c_uint32)), ("cand_excl", C.POINTER(C.c_uint32)), ("seconds_kernels", C.c_double), ("probes", C.c_uint64)]


class ExclusiveResults(C.Structure):
    _fields_ = [("n_user_bins", C.c_uint64), ("precision", C.c_uint32), ("reserved", C.c_uint32), ("cand_reads", C.POINTER(C.c_uint64)),
                ("hits", C.POINTER(C.c_uint64)), ("exclusive_hits", C.POINTER(C.c_uint64)), ("exclusive_reads", C.POINTER(C.c_uint64)),
                ("registers", C.POINTER(C.c_uint8)), ("seconds_kernels", C.c_double), ("probes", C.c_uint64)]


class CensusResults(C.Structure):
    _fields_ = [("n_ixf", C.c_uint64), ("n_bins", C.c_uint64), ("n_user_bins", C.c_uint64), ("bin_first", C.POINTER(C.c_uint64)),
                ("nonzero", C.POINTER(C.c_uint64)), ("seconds_kernel", C.c_double), ("bytes_read", C.c_uint64), ("n_tiles", C.c_uint64),
                ("launches", C.c_uint32), ("reserved", C.c_uint32)]


class HitmapBatch(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_mapped", C.c_uint64), ("segments", C.c_uint32), ("reserved", C.c_uint32),
                ("map_off", C.POINTER(C.c_uint64)), ("tuple", C.POINTER(C.c_uint64)), ("user_bin", C.POINTER(C.c_int64)),
                ("count", C.POINTER(C.c_uint32)), ("hits", C.POINTER(C.c_uint32)), ("n_hashes", C.POINTER(C.c_uint32)),
                ("seconds_kernels", C.c_double), ("probes", C.c_uint64)]


SIGNATURES = {
    "taxor_gpu_last_error": (C.c_char_p, []),
    "taxor_gpu_index_create": (C.c_int, [C.POINTER(HixfView), C.c_int, C.POINTER(_P)]),
    "taxor_gpu_index_destroy": (None, [_P]),
    "taxor_index_plan_passes": (C.c_int, [C.POINTER(HixfView), C.c_uint64, C.POINTER(PassPlan), _P, _P]),
    "taxor_gpu_index_create_paged": (C.c_int, [C.POINTER(HixfView), C.c_int, C.c_uint64, C.POINTER(_P)]),
    "taxor_gpu_index_passes": (C.c_uint32, [_P]),
    "taxor_gpu_index_load_pass": (C.c_int, [_P, C.POINTER(HixfView), C.c_uint32]),
    "taxor_gpu_index_upload_wait_seconds": (C.c_double, [_P]),
    "taxor_gpu_search_merge_prior": (C.c_int, [_P, C.POINTER(Prior), C.c_uint32]),
    "taxor_gpu_results_keys": (C.c_int, [_P, C.POINTER(C.POINTER(C.c_uint32))]),
    "taxor_gpu_search_capture": (C.c_int, [_P, C.c_int]),
    "taxor_gpu_search_take_saved": (C.c_int, [_P, C.POINTER(_P)]),
    "taxor_gpu_saved_view_get": (C.c_int, [_P, C.POINTER(SavedView)]),
    "taxor_gpu_saved_bytes": (C.c_uint64, [_P]),
    "taxor_gpu_saved_free": (None, [_P]),
    "taxor_gpu_search_capture_positions": (C.c_int, [_P, C.c_int]),
    "taxor_gpu_saved_positions": (C.c_int, [_P, C.POINTER(C.POINTER(C.c_uint32))]),
    "taxor_gpu_saved_positions_seconds": (C.c_double, [_P]),
    "taxor_gpu_search_saved_begin": (C.c_int, [_P, _P]),
    "taxor_saved_bytes_bound": (C.c_uint64, [C.c_uint64, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32]),
    "taxor_saved_store_fits": (C.c_int, [C.c_uint64, C.c_uint64]),
    "taxor_gpu_index_build_hixf": (C.c_int, [_P, _P, _P, C.c_uint64, C.POINTER(C.c_uint32)]),
    "taxor_gpu_index_build_ixf_ex": (C.c_int, [_P, C.c_uint64, _P, C.c_int, _P, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(BuildStats)]),
    "taxor_gpu_index_build_hixf_ex": (C.c_int, [_P, _P, C.c_int, _P, C.c_uint64, C.POINTER(BuildStats)]),
    "taxor_gpu_index_build_hixf_gen": (C.c_int, [_P, _P, C.c_int, _P, _P, _P, C.c_uint64, C.c_uint64, C.POINTER(BuildStats)]),
    "taxor_gpu_keys_union": (C.c_int, [C.c_int, _P, _P, C.c_uint64, C.c_int, _P, C.c_int, C.c_uint64, C.POINTER(C.c_uint64)]),
    "taxor_gpu_index_build_ixf_bins": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_uint64, _P, C.c_int, _P, C.c_uint64, C.c_uint32, C.POINTER(C.c_int)]),
    "taxor_gpu_index_build_hixf_stream": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_uint64, C.POINTER(BuildStats)]),
    "taxor_gpu_index_build_hixf_stream_ranges": (C.c_int, [_P, _P, _P, _P, C.c_uint64, C.c_uint64, C.POINTER(BuildStats)]),
    "taxor_gpu_keyer_create": (C.c_int, [C.c_int, C.POINTER(KeyerParams), C.POINTER(_P)]),
    "taxor_gpu_keyer_add": (C.c_int, [_P, _P, _P, _P, C.c_uint64]),
    "taxor_gpu_keyer_finish": (C.c_int, [_P, C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.POINTER(C.c_uint64))]),
    "taxor_gpu_keyer_union_size": (C.c_int, [_P, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "taxor_gpu_keyer_arrange": (C.c_int, [_P, _P, _P, C.c_uint64, C.POINTER(C.POINTER(C.c_uint64))]),
    "taxor_gpu_keyer_stats": (C.c_int, [_P, C.POINTER(KeyerStats)]),
    "taxor_gpu_keyer_destroy": (None, [_P]),
    "taxor_gpu_profile_create": (C.c_int, [C.c_int, C.POINTER(ProfileCsr), C.POINTER(_P)]),
    "taxor_gpu_profile_run": (C.c_int, [_P, C.c_uint32, C.c_uint32]),
    "taxor_gpu_profile_results": (C.c_int, [_P, C.POINTER(ProfileResults)]),
    "taxor_gpu_profile_destroy": (None, [_P]),
    "taxor_gpu_profile_feed_create": (C.c_int, [C.c_int, C.c_uint64, _P, _P, C.c_uint64, C.POINTER(_P)]),
    "taxor_gpu_profile_feed_add_batch": (C.c_int, [_P, _P, C.c_uint64, C.c_uint32]),
    "taxor_gpu_profile_feed_add_csr": (C.c_int, [_P, C.c_uint64, C.c_uint64, _P, _P, _P, _P, _P, C.c_uint32]),
    "taxor_gpu_profile_feed_finish": (C.c_int, [_P, _P, C.c_uint64, C.POINTER(_P)]),
    "taxor_gpu_profile_feed_matches": (C.c_int, [_P, C.POINTER(ProfileCsr), C.POINTER(C.POINTER(C.c_int64))]),
    "taxor_gpu_profile_feed_destroy": (None, [_P]),
    "taxor_gpu_coverage_create": (C.c_int, [_P, C.POINTER(HixfView), C.c_uint32, C.POINTER(_P)]),
    "taxor_gpu_coverage_add_batch": (C.c_int, [_P, _P, _P]),
    "taxor_gpu_coverage_results": (C.c_int, [_P, C.POINTER(CoverageResults)]),
    "taxor_gpu_coverage_destroy": (None, [_P]),
    "taxor_lineage_create": (C.c_int, [C.POINTER(HixfMeta), C.c_uint64, C.POINTER(_P)]),
    "taxor_lineage_get_view": (C.c_int, [_P, C.POINTER(LineageView)]),
    "taxor_lineage_free": (None, [_P]),
    "taxor_gpu_lca_create": (C.c_int, [_P, _P, C.POINTER(_P)]),
    "taxor_gpu_lca_add_batch": (C.c_int, [_P, _P, C.c_uint64, C.POINTER(LcaCalls)]),
    "taxor_gpu_lca_add_csr": (C.c_int, [_P, C.c_uint64, _P, _P, _P, _P, C.POINTER(LcaCalls)]),
    "taxor_gpu_lca_results": (C.c_int, [_P, C.POINTER(LcaResults)]),
    "taxor_gpu_lca_destroy": (None, [_P]),
    "taxor_gpu_confidence_create": (C.c_int, [_P, C.POINTER(HixfView), _P, C.c_double, C.POINTER(_P)]),
    "taxor_gpu_confidence_add_batch": (C.c_int, [_P, _P, _P, C.c_uint64, C.POINTER(ConfidenceCalls)]),
    "taxor_gpu_confidence_add_csr": (C.c_int, [_P, C.c_uint64, _P, _P, _P, _P, _P, _P, C.POINTER(ConfidenceCalls)]),
    "taxor_gpu_confidence_results": (C.c_int, [_P, C.POINTER(LcaResults)]),
    "taxor_gpu_confidence_destroy": (None, [_P]),
    "taxor_gpu_breakpoint_create": (C.c_int, [_P, C.POINTER(HixfView), C.c_uint32, C.POINTER(_P)]),
    "taxor_gpu_breakpoint_add_batch": (C.c_int, [_P, _P, _P, C.POINTER(BreakpointBatch)]),
    "taxor_gpu_breakpoint_add_csr": (C.c_int, [_P, C.c_uint64, _P, _P, _P, _P, _P, C.POINTER(BreakpointBatch)]),
    "taxor_gpu_breakpoint_destroy": (None, [_P]),
    "taxor_gpu_segments_create": (C.c_int, [_P, C.POINTER(HixfView), C.c_uint32, C.POINTER(_P)]),
    "taxor_gpu_segments_add_batch": (C.c_int, [_P, _P, _P, C.POINTER(SegmentsBatch)]),
    "taxor_gpu_segments_add_csr": (C.c_int, [_P, C.c_uint64, _P, _P, _P, _P, _P, C.POINTER(SegmentsBatch)]),
    "taxor_gpu_segments_destroy": (None, [_P]),
    "taxor_gpu_exclusive_create": (C.c_int, [_P, C.POINTER(HixfView), C.c_uint32, C.POINTER(_P)]),
    "taxor_gpu_exclusive_add_batch": (C.c_int, [_P, _P, _P, C.POINTER(ExclusiveBatch)]),
    "taxor_gpu_exclusive_add_csr": (C.c_int, [_P, C.c_uint64, _P, _P, _P, _P, _P, C.POINTER(ExclusiveBatch)]),
    "taxor_gpu_exclusive_results": (C.c_int, [_P, C.POINTER(ExclusiveResults)]),
    "taxor_gpu_exclusive_destroy": (None, [_P]),
    "taxor_gpu_census_create": (C.c_int, [_P, C.POINTER(_P)]),
    "taxor_gpu_census_run": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(CensusResults)]),
    "taxor_gpu_census_destroy": (None, [_P]),
    "taxor_census_keys_est": (C.c_uint64, [C.c_uint64]),
    "taxor_census_capacity": (C.c_uint64, [C.c_uint64]),
    "taxor_census_peeled": (C.c_int, [C.c_uint64, C.c_uint64]),
    "taxor_census_ref_line": (C.c_uint64, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_char_p, C.c_uint64]),
    "taxor_census_ixf_line": (C.c_uint64, [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_char_p, C.c_uint64]),
    "taxor_census_breadth_columns": (C.c_uint64, [C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_char_p, C.c_uint64]),
    "taxor_gpu_hitmap_create": (C.c_int, [_P, C.POINTER(HixfView), C.c_uint32, C.POINTER(_P)]),
    "taxor_gpu_hitmap_add_batch": (C.c_int, [_P, _P, _P, C.POINTER(HitmapBatch)]),
    "taxor_gpu_hitmap_destroy": (None, [_P]),
    "taxor_hll_estimate": (C.c_double, [_P, C.c_uint32]),
    "taxor_hll_slot": (None, [C.c_uint64, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)]),
    "taxor_gpu_device_memory": (C.c_int, [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "taxor_build_layout": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.POINTER(C.POINTER(Layout))]),
    "taxor_layout_free": (None, [C.POINTER(Layout)]),
    "taxor_gpu_keys_sketch": (C.c_int, [C.c_int, _P, C.c_int, _P, C.c_uint64, C.c_uint32, _P, _P]),
    "taxor_gpu_sketch_pairs": (C.c_int, [C.c_int, _P, _P, _P, C.c_uint64, C.c_uint32, _P, _P, C.POINTER(C.c_float)]),
    "taxor_cluster_order": (C.c_int, [_P, _P, C.c_uint64, C.c_double, _P, _P]),
    "taxor_similarity_rank": (C.c_int, [C.c_int, _P, _P, _P, C.c_uint64, C.c_uint32, C.c_uint64, C.c_double, _P, C.POINTER(C.c_uint64),
                                      C.POINTER(C.c_float)]),
    "taxor_build_layout_ranked": (C.c_int, [_P, C.c_uint64, C.c_uint64, _P, C.POINTER(C.POINTER(Layout))]),
    "taxor_synth_key": (C.c_uint64, [C.c_uint64, C.c_uint64]),
    "taxor_gpu_synth_keys": (C.c_int, [C.c_int, _P, C.c_uint64, C.c_uint64, C.c_uint64]),
    "taxor_gpu_malloc": (C.c_int, [C.c_int, C.c_uint64, C.POINTER(_P)]),
    "taxor_gpu_free": (None, [_P]),
    "taxor_gpu_memcpy_to_host": (C.c_int, [_P, _P, C.c_uint64]),
    "taxor_gpu_memcpy_from_host": (C.c_int, [_P, _P, C.c_uint64]),
    "taxor_gpu_index_ixf_seed": (C.c_uint64, [_P, C.c_uint64]),
    "taxor_gpu_index_data_bytes": (C.c_uint64, [_P]),
    "taxor_gpu_gather_ceiling": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "taxor_gpu_gather_ceiling_span": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64),
                                              C.POINTER(C.c_uint64)]),
    "taxor_gpu_gather_pattern": (C.c_int, [_P, C.c_uint64, C.c_int, C.c_int, C.c_uint64, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_uint64)]),
    "taxor_gpu_index_leaf_runs": (C.c_uint64, [_P]),
    "taxor_gpu_index_depth": (C.c_uint32, [_P]),
    "taxor_gpu_index_fill_random": (C.c_int, [_P, C.c_uint64, C.c_uint64]),
    "taxor_gpu_index_upload_bin": (C.c_int, [_P, C.c_uint64, C.c_uint64, _P, C.c_uint64]),
    "taxor_gpu_index_download_ixf": (C.c_int, [_P, C.c_uint64, _P, C.c_uint64]),
    "taxor_gpu_index_root_plane": (C.c_int, [_P, _P, C.c_uint64, _P, _P]),
    "taxor_gpu_index_build_ixf": (C.c_int, [_P, C.c_uint64, _P, _P, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    "taxor_gpu_searcher_create": (C.c_int, [_P, C.POINTER(SearchParams), C.POINTER(_P)]),
    "taxor_gpu_searcher_destroy": (None, [_P]),
    "taxor_threshold_kind": (C.c_int, [C.c_int, C.c_uint32, C.c_uint64, C.c_double]),
    "taxor_threshold_model": (C.c_uint64, [C.c_int, C.c_uint64, C.c_uint32, C.c_double, C.c_double, C.c_double]),
    "taxor_threshold_select": (C.c_int, [C.POINTER(HixfView), C.c_double, C.c_double, C.POINTER(SearchParams)]),
    "taxor_gpu_host_register": (C.c_int, [_P, C.c_uint64]),
    "taxor_gpu_host_unregister": (C.c_int, [_P]),
    "taxor_gpu_search_batch_begin": (C.c_int, [_P, _P, _P, C.c_uint64]),
    "taxor_gpu_search_segments_begin": (C.c_int, [_P, C.POINTER(ReadSegment), C.c_uint64]),
    "taxor_gpu_search_fastx_begin": (C.c_int, [_P, _P, C.c_uint64, C.c_int, C.POINTER(FastxScan)]),
    "taxor_gpu_search_nibbles_begin": (C.c_int, [_P, C.POINTER(NibbleSegment), C.c_uint64]),
    "taxor_gpu_pack_nibbles": (C.c_int, [_P, C.POINTER(NibbleSegment), C.c_uint64, C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.POINTER(C.c_uint32)),
                                         C.POINTER(C.c_float)]),
    "taxor_gpu_search_batch_end": (C.c_int, [_P, C.POINTER(Results)]),
    "taxor_gpu_search_batch": (C.c_int, [_P, _P, _P, C.c_uint64, C.POINTER(Results)]),
    "taxor_gpu_batch_upload": (C.c_int, [_P, _P, _P, C.c_uint64]),
    "taxor_gpu_pack_dna4_timed": (C.c_int, [_P, _P, _P, C.c_uint64, C.POINTER(C.c_float)]),
    "taxor_gpu_batch_run": (C.c_int, [_P]),
    "taxor_gpu_batch_sync": (C.c_int, [_P]),
    "taxor_gpu_batch_fetch": (C.c_int, [_P, C.POINTER(Results)]),
    "taxor_gpu_batch_result_sizes": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "taxor_gpu_batch_export_device": (C.c_int, [_P, _P, _P, _P, _P]),
    "taxor_gpu_batch_stats": (C.c_int, [_P, C.POINTER(RunStats)]),
    "taxor_gpu_comm_create": (C.c_int, [C.POINTER(C.c_int), C.c_uint32, C.c_int, C.POINTER(_P)]),
    "taxor_gpu_comm_destroy": (None, [_P]),
    "taxor_gpu_index_create_replicated": (C.c_int, [_P, C.POINTER(HixfView), C.POINTER(_P)]),
    "taxor_gpu_gather_results": (C.c_int, [_P, C.POINTER(_P), C.POINTER(Results)]),
    "taxor_gpu_comm_info": (C.c_int, [_P, C.POINTER(CommStats)]),
    "taxor_gpu_comm_set_self_exchange": (C.c_int, [_P, C.c_int]),
    # test and profiling entry points (include/taxor_gpu_tools.h)
    "taxor_gpu_phase_profile": (C.c_int, [_P, _P]),
    "taxor_gpu_syncmers": (C.c_int, [_P, _P, _P, C.c_uint64, C.POINTER(C.POINTER(C.c_uint64)),
                                     C.POINTER(C.POINTER(C.c_uint64))]),
    "taxor_gpu_ixf_bulk_count": (C.c_int, [_P, C.c_uint64, _P, C.c_uint64, _P]),
    "taxor_gpu_bulk_contains": (C.c_int, [_P, _P, C.c_uint64, C.c_uint64, C.POINTER(Results)]),
    "taxor_ixf_arith_code": (C.c_uint32, [C.POINTER(IxfVariant)]),
    "taxor_ixf_arith_decode": (None, [C.c_uint32, C.POINTER(IxfVariant)]),
    "taxor_ixf_build_bin_arith": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, _P]),
    "taxor_ixf_variant_default": (None, [C.POINTER(IxfVariant), C.c_uint64, C.c_uint64, C.c_uint64]),
    "taxor_gpu_ixf_variant_scan": (C.c_int, [C.c_int, _P, C.c_uint64, C.c_uint64, C.POINTER(IxfVariant), C.c_uint32, _P, _P, C.c_uint64, _P]),
    "taxor_ixf_layout_parse": (C.c_int, [C.c_char_p, C.POINTER(C.c_uint32)]),
    "taxor_ixf_layout_describe": (C.c_uint64, [C.c_uint32, C.c_char_p, C.c_uint64]),
    "taxor_hixf_set_layout": (C.c_int, [_P, C.c_uint32]),
    "taxor_hixf_ixf_raw_bytes": (C.c_uint64, [_P, C.c_uint64]),
    "taxor_ixf_variant_describe": (C.c_uint64, [C.POINTER(IxfVariant), C.c_char_p, C.c_uint64]),
    "taxor_hixf_load": (C.c_int, [C.c_char_p, C.POINTER(_P)]),
    "taxor_ixf_schema_default": (None, [C.POINTER(IxfSchema)]),
    "taxor_hixf_probe": (C.c_int, [C.c_char_p, C.POINTER(IxfSchema), C.c_char_p, C.c_uint64]),
    "taxor_hixf_load_schema": (C.c_int, [C.c_char_p, C.POINTER(IxfSchema), C.POINTER(_P)]),
    "taxor_hixf_store_schema": (C.c_int, [C.c_char_p, C.POINTER(HixfView), C.POINTER(HixfMeta), C.POINTER(IxfSchema)]),
    "taxor_hixf_free": (None, [_P]),
    "taxor_hixf_release_data": (None, [_P]),
    "taxor_hixf_set_arith": (None, [_P, C.c_uint32]),
    "taxor_hixf_get_view": (C.POINTER(HixfView), [_P]),
    "taxor_hixf_get_meta": (C.POINTER(HixfMeta), [_P]),
    "taxor_hixf_store": (C.c_int, [C.c_char_p, C.POINTER(HixfView), C.POINTER(HixfMeta)]),
    "taxor_format_read": (C.c_uint64, [_P, C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint32, _P, _P, C.c_uint64,
                                       _P, C.c_uint64]),
    "taxor_format_reads": (C.c_uint64, [_P, C.c_uint64, _P, _P, _P, _P, _P, _P, _P, _P, C.c_uint64]),
    "taxor_threshold_ratio": (C.c_double, [C.c_uint32, C.c_double, C.c_double]),
    "taxor_threshold": (C.c_uint64, [C.c_uint64, C.c_double]),
    "taxor_classify_filter": (None, [_P, C.c_uint64, _P]),
    "taxor_ixf_seg_len": (C.c_uint64, [C.c_uint64]),
    "taxor_ixf_build_bin": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_uint64, _P]),
    "taxor_synth_reads": (C.c_int, [_P, _P, C.c_uint64, C.c_uint64, C.c_uint32, C.c_double, C.c_double,
                                    C.c_double, C.c_uint64, C.c_int, _P, C.c_uint64, _P, _P]),
}

_lib = None


def lib():
    """Load libtaxor_gpu.so; raise loudly if it is absent (no CPU path exists in the product)."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise RuntimeError(
                f"{SO_PATH} is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; "
                "g.build()' or make -C taxor_amd/csrc).  taxor_amd has no CPU fallback.")
        L = C.CDLL(SO_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError if the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


class TaxorError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"[TAXOR SEARCH ERROR] {msg} (status {code})")
        self.code = code


def check(rc):
    if rc != 0:
        raise TaxorError(rc, lib().taxor_gpu_last_error().decode(errors="replace"))
