"""ctypes binding of include/plasship.h (no torch types cross the boundary)."""
import ctypes as C
import os
from dataclasses import dataclass

_HERE = os.path.dirname(os.path.abspath(__file__))


def lib_path():
    """the in-tree C-ABI library; PLASSHIP_LIB names another build of it (A/B runs of kernel variants)"""
    return os.environ.get("PLASSHIP_LIB") or os.path.join(_HERE, "libplasship.so")


def clust_lib_path():
    """the extension library with greedy clustering (include/plasship_ext/clust.h), beside the C-ABI library"""
    return os.path.join(os.path.dirname(lib_path()), "libplasship_clust.so")


def linclust_lib_path():
    """the extension library with linclust's ungapped alignment step (include/plasship_ext/linclust.h), beside the other two"""
    return os.path.join(os.path.dirname(lib_path()), "libplasship_linclust.so")


def subst_lib_path():
    """the extension library with linclust's diagonal filter (rescorediagonal --rescore-mode 1) and result2repseq (include/plasship_ext/subst.h),
    beside the other three"""
    return os.path.join(os.path.dirname(lib_path()), "libplasship_subst.so")


def gencode_lib_path():
    """the extension library with extractorfs / translatenucs for any genetic code (include/plasship_ext/gencode.h), beside the others"""
    return os.path.join(os.path.dirname(lib_path()), "libplasship_gencode.so")


def cc_lib_path():
    """the extension library with connected-component clustering (clust --cluster-mode 1, include/plasship_ext/cc.h), beside the others"""
    return os.path.join(os.path.dirname(lib_path()), "libplasship_cc.so")


class PlasshipError(RuntimeError):
    pass


class _KmermatchParams(C.Structure):
    _fields_ = [("kmer_size", C.c_int32), ("alphabet_size", C.c_int32), ("kmers_per_seq", C.c_int32),
                ("kmers_per_seq_scale", C.c_float), ("hash_shift", C.c_int32), ("include_only_extendable", C.c_int32),
                ("ignore_multi_kmer", C.c_int32), ("cov_mode", C.c_int32), ("cov_thr", C.c_float)]


class KmermatchStats(C.Structure):
    _fields_ = [("n_kmer_records", C.c_uint64), ("n_grouped", C.c_uint64), ("n_candidates", C.c_uint64),
                ("record_bytes", C.c_uint32), ("ms_extract", C.c_float), ("ms_sort1", C.c_float),
                ("ms_group", C.c_float), ("ms_sort2", C.c_float), ("ms_reduce", C.c_float), ("ms_extract_kernel", C.c_float),
                ("residues", C.c_uint64), ("ms_extract_short_kernel", C.c_float), ("ms_extract_wave_kernel", C.c_float),
                ("short_residues", C.c_uint64), ("short_records", C.c_uint64), ("wave_residues", C.c_uint64), ("wave_records", C.c_uint64),
                ("ms_part_scatter", C.c_float), ("n_part_scatter", C.c_int32), ("n_scratch_sequences", C.c_uint32), ("n_restarts", C.c_uint32),
                ("n_cached_sequences", C.c_uint32), ("reserved0", C.c_uint32)]


class _RescoreParams(C.Structure):
    _fields_ = [("rescore_mode", C.c_int32), ("eval_thr", C.c_double), ("seq_id_thr", C.c_float), ("cov_mode", C.c_int32),
                ("cov_thr", C.c_float), ("min_aln_len", C.c_int32), ("seq_id_mode", C.c_int32), ("add_backtrace", C.c_int32),
                ("include_identity", C.c_int32)]


class RescoreStats(C.Structure):
    _fields_ = [("n_scored", C.c_uint64), ("n_accepted", C.c_uint64), ("overlap_residues", C.c_uint64), ("ms_kernel", C.c_float)]


class _HammingParams(C.Structure):
    _fields_ = [("wrapped", C.c_int32), ("seq_id_thr", C.c_float), ("seq_id_mode", C.c_int32), ("cov_mode", C.c_int32),
                ("cov_thr", C.c_float), ("min_aln_len", C.c_int32), ("eval_thr", C.c_double)]


class _SubstParams(C.Structure):
    _fields_ = [("eval_thr", C.c_double), ("seq_id_thr", C.c_float), ("cov_thr", C.c_float), ("cov_mode", C.c_int32), ("min_aln_len", C.c_int32),
                ("score_per_col_thr", C.c_float)]


class _LocalParams(C.Structure):
    _fields_ = [("eval_thr", C.c_double), ("seq_id_thr", C.c_float), ("seq_id_mode", C.c_int32), ("cov_thr", C.c_float), ("cov_mode", C.c_int32),
                ("min_aln_len", C.c_int32), ("add_backtrace", C.c_int32), ("score_per_col_thr", C.c_float)]


class ClustStats(C.Structure):
    _fields_ = [("n_sequences", C.c_uint64), ("n_edges", C.c_uint64), ("n_clusters", C.c_uint64), ("n_promoted", C.c_uint64),
                ("n_long_queries", C.c_uint64), ("ms_kernel", C.c_float)]


class CcStats(C.Structure):
    _fields_ = [("n_sequences", C.c_uint64), ("n_edges", C.c_uint64), ("n_clusters", C.c_uint64), ("n_missing_links", C.c_uint64),
                ("n_hook_rounds", C.c_uint32), ("n_bfs_levels", C.c_uint32), ("ms_kernel", C.c_float)]


class _AssembleParams(C.Structure):
    _fields_ = [("seq_id_thr", C.c_float), ("max_seq_len", C.c_uint64), ("keep_target", C.c_int32), ("rescore_mode", C.c_int32)]


class AssembleStats(C.Structure):
    _fields_ = [("n_extended", C.c_uint64), ("n_rescored", C.c_uint64), ("out_residues", C.c_uint64), ("ms_kernel", C.c_float),
                ("ms_assemble_kernel", C.c_float), ("n_alignments", C.c_uint64), ("rescored_residues", C.c_uint64),
                ("ms_tier_kernel", C.c_float * 3), ("tier_alignments", C.c_uint64 * 3), ("tier_query_residues", C.c_uint64 * 3),
                ("tier_rescored_residues", C.c_uint64 * 3), ("db_appended_bytes", C.c_uint64), ("db_copied_bytes", C.c_uint64)]


class _Aln2NuclParams(C.Structure):
    _fields_ = [("gap_open", C.c_int32), ("gap_extend", C.c_int32)]


class Aln2NuclStats(C.Structure):
    _fields_ = [("n_alignments", C.c_uint64), ("ms_kernel", C.c_float)]


class FindStartStats(C.Structure):
    _fields_ = [("n_alignments", C.c_uint64), ("out_residues", C.c_uint64), ("ms_kernel", C.c_float)]


class _CyclecheckParams(C.Structure):
    _fields_ = [("max_seq_len", C.c_uint64), ("chop_cycle", C.c_int32)]


class CyclecheckStats(C.Structure):
    _fields_ = [("n_cyclic", C.c_uint64), ("n_wave_small", C.c_uint64), ("n_wave_large", C.c_uint64), ("n_block", C.c_uint64), ("ms_kernel", C.c_float), ("n_known", C.c_uint64)]


class _OrfParams(C.Structure):
    _fields_ = [("min_length", C.c_int32), ("max_length", C.c_int32), ("max_gaps", C.c_int32), ("contig_start_mode", C.c_int32),
                ("contig_end_mode", C.c_int32), ("orf_start_mode", C.c_int32), ("forward_frames", C.c_int32), ("reverse_frames", C.c_int32),
                ("translation_table", C.c_int32), ("translate", C.c_int32), ("use_all_table_starts", C.c_int32), ("max_seq_len", C.c_uint64)]


class _TranslateParams(C.Structure):
    _fields_ = [("translation_table", C.c_int32), ("add_orf_stop", C.c_int32), ("max_seq_len", C.c_uint64)]


class OrfStats(C.Structure):
    _fields_ = [("n_out", C.c_uint64), ("in_residues", C.c_uint64), ("out_residues", C.c_uint64), ("ms_kernel", C.c_float)]


class _SynthParams(C.Structure):
    _fields_ = [("n_pairs", C.c_uint64), ("seed", C.c_uint64), ("n_genomes", C.c_uint32), ("genome_min_len", C.c_uint64),
                ("genome_max_len", C.c_uint64), ("abundance_sigma", C.c_float), ("insert_mean", C.c_float), ("insert_sd", C.c_float),
                ("insert_min", C.c_uint32), ("read_len", C.c_uint32), ("error_rate", C.c_float)]


class SynthStats(C.Structure):
    _fields_ = [("genome_bases", C.c_uint64), ("n_genes", C.c_uint64), ("mean_coverage", C.c_double), ("max_coverage", C.c_double),
                ("ms_kernel", C.c_float)]


class _MergeParams(C.Structure):
    _fields_ = [("min_overlap", C.c_int32), ("max_overlap", C.c_int32), ("max_mismatch_density", C.c_float),
                ("cap_mismatch_quals", C.c_int32), ("allow_outies", C.c_int32)]


class MergeStats(C.Structure):
    _fields_ = [("pairs", C.c_uint64), ("combined", C.c_uint64), ("not_combined", C.c_uint64), ("long_pairs", C.c_uint64),
                ("ms_parse", C.c_float), ("ms_upload", C.c_float), ("ms_kernel", C.c_float)]


class _CreatedbParams(C.Structure):
    _fields_ = [("shuffle", C.c_int32), ("id_offset", C.c_uint32), ("dbtype", C.c_int32)]


class CreatedbStats(C.Structure):
    _fields_ = [("entries", C.c_uint64), ("files", C.c_uint64), ("chunks", C.c_uint64), ("bytes_in", C.c_uint64), ("bytes_out", C.c_uint64),
                ("lines", C.c_uint64), ("ms_read", C.c_float), ("ms_upload", C.c_float), ("ms_kernel", C.c_float), ("ms_write_kernel", C.c_float),
                ("ms_total", C.c_float)]


class _SelectParams(C.Structure):
    _fields_ = [("mode", C.c_int32), ("only_extended", C.c_int32), ("min_contig_len", C.c_int64)]


class SelectStats(C.Structure):
    _fields_ = [("n_selected", C.c_uint64), ("n_s1_only", C.c_uint64), ("n_s2_only", C.c_uint64), ("n_both", C.c_uint64),
                ("n_cycle", C.c_uint64), ("ms_kernel", C.c_float)]


class FastaStats(C.Structure):
    _fields_ = [("n_entries", C.c_uint64), ("bytes", C.c_uint64), ("n_chunks", C.c_uint64), ("ms_kernel", C.c_float), ("ms_total", C.c_float)]


class SubdbStats(C.Structure):
    _fields_ = [("n_entries", C.c_uint64), ("bytes", C.c_uint64), ("n_cycle", C.c_uint64), ("ms_kernel", C.c_float), ("ms_total", C.c_float)]


class AlnRecord(C.Structure):
    _fields_ = [("query_key", C.c_uint32), ("target_key", C.c_uint32), ("bit_score", C.c_int32), ("raw_score", C.c_int32),
                ("seq_id", C.c_float), ("q_start", C.c_int32), ("q_end", C.c_int32), ("q_len", C.c_int32),
                ("db_start", C.c_int32), ("db_end", C.c_int32), ("db_len", C.c_int32), ("aln_len", C.c_int32), ("reversed", C.c_int32)]


# every symbol include/plasship.h declares: (name, restype, argtypes)
P = C.c_void_p
SYMBOLS = [
    ("plasship_last_error", C.c_char_p, []),
    ("plasship_version", C.c_char_p, []),
    ("plasship_ctx_create", C.c_int, [C.c_int, C.POINTER(P)]),
    ("plasship_ctx_destroy", None, [P]),
    ("plasship_ctx_sync", C.c_int, [P]),
    ("plasship_ctx_reserve_async", C.c_int, [P]),
    ("plasship_ctx_stream", P, [P]),
    ("plasship_host_syncs", C.c_ulonglong, []),
    ("plasship_ctx_debug_fail_collective", C.c_int, [P, C.c_int]),
    ("plasship_ctx_set_comm", C.c_int, [P, P]),
    ("plasship_ctx_copy_d2d", C.c_int, [P, P, P, C.c_uint64]),
    ("plasship_seqdb_upload", C.c_int, [P, C.c_char_p, C.c_size_t, P, P, P, C.c_size_t, C.c_int, C.POINTER(P)]),
    ("plasship_seqdb_read", C.c_int, [P, C.c_char_p, C.POINTER(P)]),
    ("plasship_seqdb_write", C.c_int, [P, P, C.c_char_p]),
    ("plasship_seqdb_info", C.c_int, [P, C.POINTER(C.c_size_t), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_int), C.POINTER(C.c_uint64)]),
    ("plasship_seqdb_digest", C.c_int, [P, P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("plasship_seqdb_download", C.c_int, [P, P, P, P, P, P]),
    ("plasship_seqdb_free", None, [P, P]),
    ("plasship_kmermatch", C.c_int, [P, P, C.POINTER(_KmermatchParams), C.POINTER(P), C.POINTER(KmermatchStats)]),
    ("plasship_cands_write", C.c_int, [P, P, P, C.c_char_p]),
    ("plasship_cands_read", C.c_int, [P, P, P, C.c_char_p, C.POINTER(P)]),
    ("plasship_cands_count", C.c_int, [P, C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
    ("plasship_cands_download", C.c_int, [P, P, P, P, P, P, P, P]),
    ("plasship_cands_free", None, [P, P]),
    ("plasship_rescore", C.c_int, [P, P, P, P, C.POINTER(_RescoreParams), C.POINTER(P), C.POINTER(RescoreStats)]),
    ("plasship_rescore_hamming", C.c_int, [P, P, P, P, C.POINTER(_HammingParams), C.POINTER(P), C.POINTER(RescoreStats)]),
    ("plasship_alns_write", C.c_int, [P, P, C.c_char_p]),
    ("plasship_alns_read", C.c_int, [P, P, C.c_char_p, C.POINTER(P)]),
    ("plasship_alns_count", C.c_int, [P, C.POINTER(C.c_uint64)]),
    ("plasship_alns_download", C.c_int, [P, P, P]),
    ("plasship_alns_free", None, [P, P]),
    ("plasship_assemble", C.c_int, [P, P, P, C.POINTER(_AssembleParams), C.POINTER(P), C.POINTER(AssembleStats)]),
    ("plasship_guided_assemble", C.c_int, [P, P, P, P, C.POINTER(_AssembleParams), C.POINTER(P), C.POINTER(P), C.POINTER(AssembleStats)]),
    ("plasship_aln2nucl", C.c_int, [P, P, P, P, P, P, C.POINTER(_Aln2NuclParams), C.POINTER(P), C.POINTER(Aln2NuclStats)]),
    ("plasship_find_assembly_start", C.c_int, [P, P, P, C.POINTER(P), C.POINTER(FindStartStats)]),
    ("plasship_cyclecheck", C.c_int, [P, P, C.POINTER(_CyclecheckParams), C.POINTER(P), C.POINTER(P), C.POINTER(CyclecheckStats)]),
    ("plasship_extract_orfs", C.c_int, [P, P, C.POINTER(_OrfParams), C.POINTER(P), C.POINTER(P), C.POINTER(OrfStats)]),
    ("plasship_translate_nucs", C.c_int, [P, P, P, C.POINTER(_TranslateParams), C.POINTER(P), C.POINTER(OrfStats)]),
    ("plasship_seqdb_concat", C.c_int, [P, P, P, C.POINTER(P)]),
    ("plasship_seqdb_concat_keys", C.c_int, [P, P, P, C.c_int, C.POINTER(P)]),
    ("plasship_orfhdr_concat", C.c_int, [P, P, P, C.POINTER(P)]),
    ("plasship_orfhdr_read", C.c_int, [P, C.c_char_p, C.POINTER(P)]),
    ("plasship_orfhdr_write", C.c_int, [P, P, C.c_char_p]),
    ("plasship_orfhdr_count", C.c_int, [P, C.POINTER(C.c_size_t)]),
    ("plasship_orfhdr_free", None, [P, P]),
    ("plasship_mergereads", C.c_int, [P, C.POINTER(C.c_char_p), C.c_size_t, C.POINTER(_MergeParams), C.POINTER(P), C.POINTER(P), C.POINTER(MergeStats)]),
    ("plasship_createdb", C.c_int, [P, C.POINTER(C.c_char_p), C.c_size_t, C.POINTER(_CreatedbParams), C.POINTER(P), C.POINTER(CreatedbStats)]),
    ("plasship_createdb_write", C.c_int, [P, C.POINTER(C.c_char_p), C.c_size_t, C.POINTER(_CreatedbParams), C.c_char_p, C.POINTER(P), C.POINTER(CreatedbStats)]),
    ("plasship_select_contigs", C.c_int, [P, P, P, P, C.POINTER(_SelectParams), C.POINTER(P), C.POINTER(SelectStats)]),
    ("plasship_fasta_write", C.c_int, [P, P, P, C.c_char_p, C.POINTER(FastaStats)]),
    ("plasship_subdb_write", C.c_int, [P, P, P, C.c_char_p, C.POINTER(SubdbStats)]),
]
# include/plasship_ext/clust.h (the extension library libplasship_clust.so: linclust's greedy clustering and pre-cluster subset)
CLUST_SYMBOLS = [
    ("plasship_clust_greedy_cands", C.c_int, [P, P, P, C.POINTER(P), C.POINTER(ClustStats)]),
    ("plasship_clust_greedy_alns", C.c_int, [P, P, P, C.POINTER(P), C.POINTER(ClustStats)]),
    ("plasship_clusters_count", C.c_int, [P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("plasship_clusters_download", C.c_int, [P, P, P, P, P]),
    ("plasship_clusters_write", C.c_int, [P, P, P, C.c_char_p]),
    ("plasship_clusters_free", None, [P, P]),
    ("plasship_cands_filter", C.c_int, [P, P, P, C.POINTER(P)]),
]
# include/plasship_ext/linclust.h (the extension library libplasship_linclust.so: linclust's ungapped alignment step)
LINCLUST_SYMBOLS = [
    ("plasship_rescore_local", C.c_int, [P, P, P, C.POINTER(_LocalParams), C.POINTER(P), C.POINTER(RescoreStats)]),
    ("plasship_rescore_local_subset", C.c_int, [P, P, P, P, C.POINTER(_LocalParams), C.POINTER(P), C.POINTER(RescoreStats)]),
    ("plasship_clusters_merge", C.c_int, [P, P, P, P, C.POINTER(P)]),
    ("plasship_merged_count", C.c_int, [P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("plasship_merged_download", C.c_int, [P, P, P, P, P]),
    ("plasship_merged_write", C.c_int, [P, P, P, C.c_char_p]),
    ("plasship_merged_free", None, [P, P]),
    ("plasship_clusters_read", C.c_int, [P, P, C.c_char_p, C.POINTER(P)]),
]
# include/plasship_ext/subst.h (the extension library libplasship_subst.so: linclust's diagonal filter of the protein workflow, result2repseq)
SUBST_SYMBOLS = [
    ("plasship_rescore_subst", C.c_int, [P, P, P, C.POINTER(_SubstParams), C.POINTER(P), C.POINTER(RescoreStats)]),
    ("plasship_rescore_subst_subset", C.c_int, [P, P, P, P, C.POINTER(_SubstParams), C.POINTER(P), C.POINTER(RescoreStats)]),
    ("plasship_clusters_repseqs", C.c_int, [P, P, P, C.POINTER(P)]),
    ("plasship_merged_repseqs", C.c_int, [P, P, P, C.POINTER(P)]),
]
# include/plasship_ext/cc.h (the extension library libplasship_cc.so: connected-component clustering)
CC_SYMBOLS = [
    ("plasship_clust_connected_cands", C.c_int, [P, P, P, C.c_int, C.POINTER(P), C.POINTER(CcStats)]),
    ("plasship_clust_connected_alns", C.c_int, [P, P, P, C.c_int, C.POINTER(P), C.POINTER(CcStats)]),
]
# include/plasship_ext/gencode.h (the extension library libplasship_gencode.so: extractorfs / translatenucs with any genetic code)
GENCODE_SYMBOLS = [
    ("plasship_extract_orfs_gc", C.c_int, [P, P, C.POINTER(_OrfParams), C.POINTER(P), C.POINTER(P), C.POINTER(OrfStats)]),
    ("plasship_translate_nucs_gc", C.c_int, [P, P, P, C.POINTER(_TranslateParams), C.POINTER(P), C.POINTER(OrfStats)]),
    ("plasship_gencode_info", C.c_int, [C.c_int, C.c_char_p, C.c_char_p]),
]
# include/plasship_rccl.h (native RCCL communicator of a sharded run)
RCCL_SYMBOLS = [
    ("plasship_rccl_get_unique_id", C.c_int, [P]),
    ("plasship_rccl_comm_create", C.c_int, [P, C.c_int, C.c_int, P, C.POINTER(P)]),
    ("plasship_rccl_comm_stats", C.c_int, [P, C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.c_int]),
    ("plasship_rccl_comm_destroy", None, [P, P]),
]
# include/plasship_synth.h (measurement infrastructure: synthetic read sets generated on the GPU)
SYNTH_SYMBOLS = [
    ("plasship_synth_read_pairs", C.c_int, [P, C.POINTER(_SynthParams), C.POINTER(P), C.POINTER(SynthStats)]),
]

_lib = None


def load_library():
    """dlopen the in-tree HIP library and bind every declared symbol; raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise PlasshipError("%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                            "(plass_amd has no CPU fallback)" % path)
    lib = C.CDLL(path)
    for name, res, args in SYMBOLS + SYNTH_SYMBOLS + RCCL_SYMBOLS:
        fn = getattr(lib, name)          # AttributeError if the export is missing
        fn.restype = res
        fn.argtypes = args
    # the extension library beside it (greedy clustering): its entry points are reached as lib.clust.<name>
    cpath = clust_lib_path()
    if not os.path.exists(cpath):
        raise PlasshipError("%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`" % cpath)
    lib.clust = C.CDLL(cpath)
    for name, res, args in CLUST_SYMBOLS:
        fn = getattr(lib.clust, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def load_linclust_library():
    """the extension library with linclust's ungapped alignment step, loaded when it is first asked for (Context.rescore_local), so that
    callers of the other two libraries do not depend on it: its entry points are then reached as load_library().linclust.<name>.  A missing
    library is an error, there is no fall-back."""
    lib = load_library()
    if getattr(lib, "linclust", None) is None:
        lpath = linclust_lib_path()
        if not os.path.exists(lpath):
            raise PlasshipError("%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`" % lpath)
        ext = C.CDLL(lpath)
        for name, res, args in LINCLUST_SYMBOLS:
            fn = getattr(ext, name)
            fn.restype = res
            fn.argtypes = args
        lib.linclust = ext
    return lib.linclust


def load_subst_library():
    """the extension library with linclust's diagonal filter and result2repseq, loaded when it is first asked for (Context.rescore_subst,
    Context.repseqs) behind the other three: its entry points are then reached as load_library().subst.<name>.  A missing library is an
    error, there is no fall-back."""
    lib = load_library()
    if getattr(lib, "subst", None) is None:
        load_linclust_library()
        spath = subst_lib_path()
        if not os.path.exists(spath):
            raise PlasshipError("%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`" % spath)
        ext = C.CDLL(spath)
        for name, res, args in SUBST_SYMBOLS:
            fn = getattr(ext, name)
            fn.restype = res
            fn.argtypes = args
        lib.subst = ext
    return lib.subst


def load_cc_library():
    """the extension library with connected-component clustering, loaded when it is first asked for (Context.clust_connected) behind the
    library it takes its handles from: its entry points are then reached as load_library().cc.<name>.  A missing library is an error, there
    is no fall-back."""
    lib = load_library()
    if getattr(lib, "cc", None) is None:
        cpath = cc_lib_path()
        if not os.path.exists(cpath):
            raise PlasshipError("%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`" % cpath)
        ext = C.CDLL(cpath)
        for name, res, args in CC_SYMBOLS:
            fn = getattr(ext, name)
            fn.restype = res
            fn.argtypes = args
        lib.cc = ext
    return lib.cc


def load_gencode_library():
    """the extension library with the other genetic codes, loaded when it is first asked for (Context.extractorfs_gencode, gencode_info) behind
    the library it takes its handles from: its entry points are then reached as load_library().gencode.<name>.  A missing library is an error,
    there is no fall-back."""
    lib = load_library()
    if getattr(lib, "gencode", None) is None:
        gpath = gencode_lib_path()
        if not os.path.exists(gpath):
            raise PlasshipError("%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`" % gpath)
        ext = C.CDLL(gpath)
        for name, res, args in GENCODE_SYMBOLS:
            fn = getattr(ext, name)
            fn.restype = res
            fn.argtypes = args
        lib.gencode = ext
    return lib.gencode


def gencode_info(table):
    """(residues, starts) of --translation-table `table`: two 64-letter strings over the codons in T, C, A, G order; an id the reference does not
    accept raises"""
    res, sta = C.create_string_buffer(65), C.create_string_buffer(65)
    _check(load_gencode_library().plasship_gencode_info(int(table), res, sta), "plasship_gencode_info")
    return res.value.decode(), sta.value.decode()


def resume_point(dir, num_iterations, name="assembly_"):
    """where `plass-hip assemble-chain / nuclassemble-chain --write-intermediate dir --resume 1 --num-iterations num_iterations` would go on:
    the highest i < num_iterations for which dir/assembly_<i>.done and the DB it vouches for (data, .index, .dbtype) exist — the run continues
    at iteration i + 1 — or None for a fresh run.  The rule of resumePoint() in csrc/cli_main.cpp; pure Python, no GPU."""
    for i in range(int(num_iterations) - 1, -1, -1):
        p = os.path.join(str(dir), "%s%d" % (name, i))
        if all(os.path.isfile(p + s) for s in (".done", "", ".index", ".dbtype")):
            return i
    return None


def _check(rc, what):
    if rc != 0:
        msg = load_library().plasship_last_error()
        raise PlasshipError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else "?"))


@dataclass
class KmermatchParams:
    """kmermatcher flags (defaults = plass assemble, src/workflow/Assembler.cpp:10-27)."""
    k: int = 14
    alph_size: int = 13
    kmer_per_seq: int = 60
    kmer_per_seq_scale: float = 0.0
    hash_shift: int = 67
    include_only_extendable: bool = False
    ignore_multi_kmer: bool = True
    cov_mode: int = 0
    c: float = 0.0

    def _c(self):
        return _KmermatchParams(self.k, self.alph_size, self.kmer_per_seq, self.kmer_per_seq_scale, self.hash_shift,
                                int(self.include_only_extendable), int(self.ignore_multi_kmer), self.cov_mode, self.c)


@dataclass
class RescoreParams:
    rescore_mode: int = 3
    e: float = 1e-5
    min_seq_id: float = 0.9
    cov_mode: int = 0
    c: float = 0.0
    min_aln_len: int = 0
    seq_id_mode: int = 0
    a: bool = False
    add_self_matches: bool = False

    def _c(self):
        return _RescoreParams(self.rescore_mode, self.e, self.min_seq_id, self.cov_mode, self.c, self.min_aln_len,
                              self.seq_id_mode, int(self.a), int(self.add_self_matches))


@dataclass
class AssembleParams:
    min_seq_id: float = 0.9
    max_seq_len: int = 65535
    keep_target: bool = True
    rescore_mode: int = 3

    def _c(self):
        return _AssembleParams(self.min_seq_id, self.max_seq_len, int(self.keep_target), self.rescore_mode)


@dataclass
class OrfParams:
    """extractorfs flags; defaults = the module's own (mm/commons/Parameters.cpp), frames as the reference's "1,2,3" lists"""
    min_length: int = 30
    max_length: int = 32734
    max_gaps: int = 2147483647
    contig_start_mode: int = 2
    contig_end_mode: int = 2
    orf_start_mode: int = 1
    forward_frames: str = "1,2,3"
    reverse_frames: str = "1,2,3"
    translation_table: int = 1
    translate: bool = False
    use_all_table_starts: bool = False
    max_seq_len: int = 65535

    @staticmethod
    def _frames(v):
        m = 0
        for f in str(v).split(","):
            f = f.strip()
            if f:
                m |= 1 << (int(f) - 1)
        return m

    def _c(self):
        return _OrfParams(self.min_length, self.max_length, self.max_gaps, self.contig_start_mode, self.contig_end_mode, self.orf_start_mode,
                          self._frames(self.forward_frames), self._frames(self.reverse_frames), self.translation_table, int(self.translate),
                          int(self.use_all_table_starts), self.max_seq_len)


# the two extractorfs passes of `plass assemble` (src/workflow/Assembler.cpp:116-130; data/assemble.sh:41-63)
PLASS_ORFS_LONG = dict(min_length=45, max_length=32734, max_gaps=0, contig_start_mode=2, contig_end_mode=2, orf_start_mode=0)
PLASS_ORFS_START = dict(min_length=20, max_length=45, max_gaps=0, contig_start_mode=1, contig_end_mode=0, orf_start_mode=0)


@dataclass
class SynthParams:
    """synthetic community + read pairs (include/plasship_synth.h)"""
    n_pairs: int = 500000
    seed: int = 1
    n_genomes: int = 1
    genome_min_len: int = 7500000
    genome_max_len: int = 7500000
    abundance_sigma: float = 0.0
    insert_mean: float = 320.0
    insert_sd: float = 40.0
    insert_min: int = 160
    read_len: int = 150
    error_rate: float = 0.002

    def _c(self):
        return _SynthParams(self.n_pairs, self.seed, self.n_genomes, self.genome_min_len, self.genome_max_len, self.abundance_sigma,
                            self.insert_mean, self.insert_sd, self.insert_min, self.read_len, self.error_rate)


@dataclass
class MergeParams:
    """the FLASH parameters of the reference's mergereads (src/assembler/mergereads.cpp:19-23); only these values are implemented"""
    min_overlap: int = 15
    max_overlap: int = 65
    max_mismatch_density: float = 0.10
    cap_mismatch_quals: bool = False
    allow_outies: bool = False

    def _c(self):
        return _MergeParams(self.min_overlap, self.max_overlap, self.max_mismatch_density, int(self.cap_mismatch_quals), int(self.allow_outies))


class Context:
    """One GPU (one process per GPU; LOCAL_RANK picks the device when ordinal < 0)."""

    def __init__(self, device=-1):
        self.lib = load_library()
        self.h = P()
        _check(self.lib.plasship_ctx_create(device, C.byref(self.h)), "plasship_ctx_create")

    def close(self):
        if self.h:
            self.lib.plasship_ctx_destroy(self.h)
            self.h = P()

    def sync(self):
        _check(self.lib.plasship_ctx_sync(self.h), "plasship_ctx_sync")

    def host_syncs(self):
        """host waits for a stream since the library was loaded (diagnostic; bench.py reports the count per iteration)"""
        return int(self.lib.plasship_host_syncs())

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- modules -------------------------------------------------------------------------------
    def read_seqdb(self, path):
        h = P()
        _check(self.lib.plasship_seqdb_read(self.h, os.fsencode(path), C.byref(h)), "plasship_seqdb_read")
        return SeqDB(self, h)

    def upload_seqdb(self, data, off, elen, key, dbtype=0):
        import numpy as np
        data = bytes(data)
        off = np.ascontiguousarray(off, dtype=np.uint64); elen = np.ascontiguousarray(elen, dtype=np.uint32)
        key = np.ascontiguousarray(key, dtype=np.uint32)
        h = P()
        _check(self.lib.plasship_seqdb_upload(self.h, data, len(data), off.ctypes.data, elen.ctypes.data, key.ctypes.data,
                                              len(key), dbtype, C.byref(h)), "plasship_seqdb_upload")
        return SeqDB(self, h)

    def kmermatcher(self, db, par=None):
        par = par or KmermatchParams()
        h = P(); st = KmermatchStats(); cp = par._c()
        _check(self.lib.plasship_kmermatch(self.h, db.h, C.byref(cp), C.byref(h), C.byref(st)), "plasship_kmermatch")
        return Candidates(self, h, db, db), st

    def read_prefdb(self, qdb, tdb, path):
        h = P()
        _check(self.lib.plasship_cands_read(self.h, qdb.h, tdb.h, os.fsencode(path), C.byref(h)), "plasship_cands_read")
        return Candidates(self, h, qdb, tdb)

    def rescorediagonal(self, qdb, tdb, cands, par=None):
        par = par or RescoreParams()
        h = P(); st = RescoreStats(); cp = par._c()
        _check(self.lib.plasship_rescore(self.h, qdb.h, tdb.h, cands.h, C.byref(cp), C.byref(h), C.byref(st)), "plasship_rescore")
        return Alignments(self, h, qdb, tdb), st

    def rescore_hamming(self, qdb, tdb, cands, wrapped=True, min_seq_id=0.0, seq_id_mode=0, cov_mode=0, c=0.0, min_aln_len=0, e=1e-3):
        """`rescorediagonal --rescore-mode 0` (the Hamming score; wrapped: --wrapped-scoring 1, the circular query of linclust's
        pre-clustering call) on a candidate list -> (the kept lines as Candidates, RescoreStats).  Defaults = the reference module's,
        except `wrapped`; linclust passes min_seq_id=0.97, cov_mode=1, c=0.99"""
        h = P(); st = RescoreStats()
        cp = _HammingParams(int(bool(wrapped)), min_seq_id, seq_id_mode, cov_mode, c, min_aln_len, e)
        _check(self.lib.plasship_rescore_hamming(self.h, qdb.h, tdb.h, cands.h, C.byref(cp), C.byref(h), C.byref(st)), "plasship_rescore_hamming")
        return Candidates(self, h, qdb, tdb), st

    def rescore_local(self, db, cands, min_seq_id=0.0, seq_id_mode=0, cov_mode=0, c=0.0, min_aln_len=0, e=1e-3, a=False, score_per_col_thr=None, subset=None):
        """`rescorediagonal --rescore-mode 2` (the best-scoring ungapped local segment on the diagonal: linclust's alignment step with
        --alignment-mode 4) on a candidate list made on `db` -> (Alignments, RescoreStats).  Defaults = the reference module's.
        score_per_col_thr: None is --filter-hits 0; a number is --filter-hits 1 with that score-per-column threshold (the reference reads
        it from a table in its binary; 0.0 is its "no row found" case).  subset: a Clusters of `db` — the call is linclust's, on the subset DB
        of its representatives (`cands` is filter_cands' list): the E-value's database size is the representatives' residue count"""
        h = P(); st = RescoreStats()
        cp = _LocalParams(e, min_seq_id, seq_id_mode, c, cov_mode, min_aln_len, int(bool(a)), float("nan") if score_per_col_thr is None else score_per_col_thr)
        if subset is not None:
            _check(load_linclust_library().plasship_rescore_local_subset(self.h, db.h, cands.h, subset.h, C.byref(cp), C.byref(h), C.byref(st)), "plasship_rescore_local_subset")
            return Alignments(self, h, db, db), st
        _check(load_linclust_library().plasship_rescore_local(self.h, db.h, cands.h, C.byref(cp), C.byref(h), C.byref(st)), "plasship_rescore_local")
        return Alignments(self, h, db, db), st

    def rescore_subst(self, db, cands, min_seq_id=0.0, cov_mode=0, c=0.0, min_aln_len=0, e=1e-3, score_per_col_thr=None, subset=None):
        """`rescorediagonal --rescore-mode 1` (the best local score on the diagonal, no positions: the filter step linclust runs on amino-acid
        DBs) on a candidate list made on `db` -> (the kept lines as Candidates, RescoreStats).  Defaults = the reference module's.
        score_per_col_thr and subset: as in rescore_local"""
        h = P(); st = RescoreStats()
        cp = _SubstParams(e, min_seq_id, c, cov_mode, min_aln_len, float("nan") if score_per_col_thr is None else score_per_col_thr)
        if subset is not None:
            _check(load_subst_library().plasship_rescore_subst_subset(self.h, db.h, cands.h, subset.h, C.byref(cp), C.byref(h), C.byref(st)), "plasship_rescore_subst_subset")
        else:
            _check(load_subst_library().plasship_rescore_subst(self.h, db.h, cands.h, C.byref(cp), C.byref(h), C.byref(st)), "plasship_rescore_subst")
        return Candidates(self, h, db, db), st

    def repseqs(self, clusters, db=None):
        """`result2repseq`: the representatives' sequences of a Clusters or MergedClusters of `db`, under their keys -> SeqDB"""
        h = P()
        db = db or clusters.db
        if isinstance(clusters, MergedClusters):
            _check(load_subst_library().plasship_merged_repseqs(self.h, clusters.h, db.h, C.byref(h)), "plasship_merged_repseqs")
        else:
            _check(load_subst_library().plasship_clusters_repseqs(self.h, clusters.h, db.h, C.byref(h)), "plasship_clusters_repseqs")
        return SeqDB(self, h)

    def clust_greedy(self, db, cands_or_alns):
        """`clust --cluster-mode 2 | 3` (greedy incremental clustering: the longest sequence that lists a sequence represents it) on a
        candidate list or an alignment list made on `db` -> (Clusters, ClustStats)"""
        h = P(); st = ClustStats()
        if isinstance(cands_or_alns, Alignments):
            _check(self.lib.clust.plasship_clust_greedy_alns(self.h, db.h, cands_or_alns.h, C.byref(h), C.byref(st)), "plasship_clust_greedy_alns")
        else:
            _check(self.lib.clust.plasship_clust_greedy_cands(self.h, db.h, cands_or_alns.h, C.byref(h), C.byref(st)), "plasship_clust_greedy_cands")
        return Clusters(self, h, db), st

    def clust_connected(self, db, cands_or_alns, max_iterations=1000):
        """`clust --cluster-mode 1` (connected component: the components of the list, each under its member with the largest symmetric list,
        ties to the shorter sequence and then the larger key) on a candidate list or an alignment list made on `db` -> (Clusters, CcStats).
        max_iterations: --max-iterations, the reference's default; where a sequence lies more than max_iterations + 1 steps from its
        representative the reference's answer depends on its visiting order and the call raises (PLASSHIP_ERR_UNSUPPORTED)"""
        h = P(); st = CcStats()
        ext = load_cc_library()
        if isinstance(cands_or_alns, Alignments):
            _check(ext.plasship_clust_connected_alns(self.h, db.h, cands_or_alns.h, int(max_iterations), C.byref(h), C.byref(st)), "plasship_clust_connected_alns")
        else:
            _check(ext.plasship_clust_connected_cands(self.h, db.h, cands_or_alns.h, int(max_iterations), C.byref(h), C.byref(st)), "plasship_clust_connected_cands")
        return Clusters(self, h, db), st

    def read_clusters(self, db, path):
        """a cluster DB (dbtype 6) from disk as a clustering of `db`, by key; a sequence the DB does not list is its own cluster (a
        clustering made on a subset DB, as linclust's second one) -> Clusters"""
        h = P()
        _check(load_linclust_library().plasship_clusters_read(self.h, db.h, os.fsencode(path), C.byref(h)), "plasship_clusters_read")
        return Clusters(self, h, db)

    def merge_clusters(self, db, first, second):
        """`mergeclusters` with two clusterings of `db`: the second clusters the first one's representatives again -> MergedClusters"""
        h = P()
        _check(load_linclust_library().plasship_clusters_merge(self.h, db.h, first.h, second.h, C.byref(h)), "plasship_clusters_merge")
        return MergedClusters(self, h, db)

    def filter_cands(self, cands, clusters):
        """what linclust's createsubdb + filterdb leave of a candidate list: the representatives' entries, and in them the lines whose
        target is a representative -> Candidates (write() writes the representatives' entries only)"""
        h = P()
        _check(self.lib.clust.plasship_cands_filter(self.h, cands.h, clusters.h, C.byref(h)), "plasship_cands_filter")
        return Candidates(self, h, cands.qdb, cands.tdb)

    def read_alndb(self, db, path):
        h = P()
        _check(self.lib.plasship_alns_read(self.h, db.h, os.fsencode(path), C.byref(h)), "plasship_alns_read")
        return Alignments(self, h, db, db)

    def assembleresults(self, db, alns, par=None):
        par = par or AssembleParams()
        h = P(); st = AssembleStats(); cp = par._c()
        _check(self.lib.plasship_assemble(self.h, db.h, alns.h, C.byref(cp), C.byref(h), C.byref(st)), "plasship_assemble")
        return SeqDB(self, h), st

    def guidedassembleresults(self, nucl_db, aa_db, alns, par=None):
        """(nuclDB, aaDB, nucleotide-level alignments) -> (nuclDB', aaDB'); reference module guidedassembleresults"""
        par = par or AssembleParams(min_seq_id=0.99, max_seq_len=200000)
        hn = P(); ha = P(); st = AssembleStats(); cp = par._c()
        _check(self.lib.plasship_guided_assemble(self.h, nucl_db.h, aa_db.h, alns.h, C.byref(cp), C.byref(hn), C.byref(ha), C.byref(st)), "plasship_guided_assemble")
        return SeqDB(self, hn), SeqDB(self, ha), st

    def proteinaln2nucl(self, nucl_db, aa_db, alns, gap_open=5, gap_extend=2):
        """protein alignments (with backtrace) of aa_db onto the nucleotide twins in nucl_db; reference module proteinaln2nucl"""
        h = P(); st = Aln2NuclStats(); cp = _Aln2NuclParams(gap_open, gap_extend)
        _check(self.lib.plasship_aln2nucl(self.h, nucl_db.h, nucl_db.h, aa_db.h, aa_db.h, alns.h, C.byref(cp), C.byref(h), C.byref(st)), "plasship_aln2nucl")
        return Alignments(self, h, nucl_db, nucl_db), st

    def findassemblystart(self, db, alns):
        """(protein DB, its alignments) -> DB with the consensus "*M" starts cut in; reference module findassemblystart,
        run once inside iteration 0 of `plass assemble` (data/assemble.sh:110-141)"""
        h = P(); st = FindStartStats()
        _check(self.lib.plasship_find_assembly_start(self.h, db.h, alns.h, C.byref(h), C.byref(st)), "plasship_find_assembly_start")
        return SeqDB(self, h), st

    def cyclecheck(self, db, max_seq_len=200000, chop_cycle=False, with_rest=False):
        """nucleotide DB -> DB of the circular / terminally redundant contigs (and, with_rest, the DB of all others);
        reference module cyclecheck, run after every nuclassembleresults of the penguin workflows"""
        hc = P(); hr = P(); st = CyclecheckStats(); cp = _CyclecheckParams(max_seq_len, int(chop_cycle))
        _check(self.lib.plasship_cyclecheck(self.h, db.h, C.byref(cp), C.byref(hc), C.byref(hr) if with_rest else None, C.byref(st)), "plasship_cyclecheck")
        return (SeqDB(self, hc), SeqDB(self, hr), st) if with_rest else (SeqDB(self, hc), st)

    # ---- row N2: the once-per-run preprocessing (data/assemble.sh:41-77) ------------------------------------------
    def extractorfs(self, reads, par=None):
        """nucleotide DB -> (ORF DB, its header DB); reference module extractorfs"""
        par = par or OrfParams()
        h = P(); hh = P(); st = OrfStats(); cp = par._c()
        _check(self.lib.plasship_extract_orfs(self.h, reads.h, C.byref(cp), C.byref(h), C.byref(hh), C.byref(st)), "plasship_extract_orfs")
        return SeqDB(self, h), OrfHeaders(self, hh), st

    def translatenucs(self, orfs, hdr=None, add_orf_stop=False, max_seq_len=65535):
        """nucleotide ORF DB (+ header DB for --add-orf-stop) -> protein DB; reference module translatenucs"""
        h = P(); st = OrfStats(); cp = _TranslateParams(1, int(add_orf_stop), max_seq_len)
        _check(self.lib.plasship_translate_nucs(self.h, orfs.h, hdr.h if hdr is not None else None, C.byref(cp), C.byref(h), C.byref(st)), "plasship_translate_nucs")
        return SeqDB(self, h), st

    def extractorfs_gencode(self, reads, par=None):
        """extractorfs with any --translation-table the reference accepts and --use-all-table-starts (libplasship_gencode.so)"""
        par = par or OrfParams()
        h = P(); hh = P(); st = OrfStats(); cp = par._c()
        _check(load_gencode_library().plasship_extract_orfs_gc(self.h, reads.h, C.byref(cp), C.byref(h), C.byref(hh), C.byref(st)), "plasship_extract_orfs_gc")
        return SeqDB(self, h), OrfHeaders(self, hh), st

    def translatenucs_gencode(self, orfs, hdr=None, add_orf_stop=False, max_seq_len=65535, translation_table=1):
        """translatenucs with any --translation-table the reference accepts (libplasship_gencode.so)"""
        h = P(); st = OrfStats(); cp = _TranslateParams(int(translation_table), int(add_orf_stop), max_seq_len)
        _check(load_gencode_library().plasship_translate_nucs_gc(self.h, orfs.h, hdr.h if hdr is not None else None, C.byref(cp), C.byref(h), C.byref(st)), "plasship_translate_nucs_gc")
        return SeqDB(self, h), st

    def concatdbs(self, a, b, preserve_keys=False):
        """reference module concatdbs (keys of A kept, B renumbered behind them; preserve_keys: B's kept as well — the union); sequence DBs or header DBs"""
        h = P()
        if preserve_keys:
            _check(self.lib.plasship_seqdb_concat_keys(self.h, a.h, b.h, 1, C.byref(h)), "plasship_seqdb_concat_keys")
            return SeqDB(self, h)
        if isinstance(a, OrfHeaders):
            _check(self.lib.plasship_orfhdr_concat(self.h, a.h, b.h, C.byref(h)), "plasship_orfhdr_concat")
            return OrfHeaders(self, h)
        _check(self.lib.plasship_seqdb_concat(self.h, a.h, b.h, C.byref(h)), "plasship_seqdb_concat")
        return SeqDB(self, h)

    def read_orfhdr(self, path):
        h = P()
        _check(self.lib.plasship_orfhdr_read(self.h, os.fsencode(path), C.byref(h)), "plasship_orfhdr_read")
        return OrfHeaders(self, h)

    def plass_fragments(self, reads, keep=False, translation_table=1, use_all_table_starts=False):
        """the whole preprocessing chain of `plass assemble` on a read DB: two extractorfs passes, translatenucs --add-orf-stop,
        concatdbs -> aa_6f_start_long, the DB iteration 0 starts from (data/assemble.sh:41-77).  Another genetic code than the standard
        one with ATG (plass assemble --translation-table N --use-all-table-starts 1) goes through the *_gencode entry points"""
        if translation_table == 1 and not use_all_table_starts:
            code, extract, translate = {}, self.extractorfs, self.translatenucs
        else:
            code, extract = dict(translation_table=translation_table, use_all_table_starts=bool(use_all_table_starts)), self.extractorfs_gencode
            translate = lambda o, h, add_orf_stop: self.translatenucs_gencode(o, h, add_orf_stop=add_orf_stop, translation_table=translation_table)      # noqa: E731
        o_long, h_long, _ = extract(reads, OrfParams(**PLASS_ORFS_LONG, **code))
        aa_long, _ = translate(o_long, h_long, add_orf_stop=True)
        o_long.free(); h_long.free()
        o_start, h_start, _ = extract(reads, OrfParams(**PLASS_ORFS_START, **code))
        aa_start, _ = translate(o_start, h_start, add_orf_stop=True)
        o_start.free(); h_start.free()
        out = self.concatdbs(aa_long, aa_start)
        aa_long.free(); aa_start.free()
        return out

    def penguin_guided_inputs(self, reads):
        """the preprocessing of `penguin guided_nuclassemble` on a read DB (data/guidedNuclAssemble.sh:44-75): two extractorfs passes,
        concatdbs of the ORFs and of their headers, translatenucs --add-orf-stop -> (nucl_6f_start_long, aa_6f_start_long)"""
        o_long, h_long, _ = self.extractorfs(reads, OrfParams(**PLASS_ORFS_LONG))
        o_start, h_start, _ = self.extractorfs(reads, OrfParams(**PLASS_ORFS_START))
        nucl = self.concatdbs(o_long, o_start)
        hdr = self.concatdbs(h_long, h_start)
        for x in (o_long, o_start, h_long, h_start):
            x.free()
        aa, _ = self.translatenucs(nucl, hdr, add_orf_stop=True)
        hdr.free()
        return nucl, aa

    def mergereads(self, paths, par=None):
        """paired-end FASTQ files [r1, r2, r1b, r2b, ...] (plain or .gz) -> (read DB, header DB, MergeStats); reference module mergereads"""
        paths = [os.fsencode(str(p)) for p in paths]
        arr = (C.c_char_p * len(paths))(*paths)
        h = P(); hh = P(); st = MergeStats(); cp = (par or MergeParams())._c()
        _check(self.lib.plasship_mergereads(self.h, arr, len(paths), C.byref(cp), C.byref(h), C.byref(hh), C.byref(st)), "plasship_mergereads")
        return SeqDB(self, h), SeqDB(self, hh), st

    def createdb(self, files, shuffle=True, id_offset=0, dbtype=0, out=None):
        """unpaired read files (FASTQ or FASTA, plain or .gz) -> (read DB, CreatedbStats); reference module createdb as the workflows run it
        on single-end input (lib/mmseqs/src/util/createdb.cpp).  `out`: also write <out>, <out>_h, <out>.lookup and <out>.source"""
        files = [os.fsencode(str(p)) for p in files]
        arr = (C.c_char_p * len(files))(*files)
        h = P(); st = CreatedbStats(); cp = _CreatedbParams(1 if shuffle else 0, int(id_offset), int(dbtype))
        if out is None:
            _check(self.lib.plasship_createdb(self.h, arr, len(files), C.byref(cp), C.byref(h), C.byref(st)), "plasship_createdb")
        else:
            _check(self.lib.plasship_createdb_write(self.h, arr, len(files), C.byref(cp), os.fsencode(str(out)), C.byref(h), C.byref(st)),
                   "plasship_createdb_write")
        return SeqDB(self, h), st

    def select_contigs(self, result, source, mode, cycles=None, only_extended=True, min_contig_len=1000):
        """the workflows' `_only_assembled` selection (data/assemble.sh:170-189 with --filter-proteins 0, data/nuclassemble.sh:151-169)
        -> (subset DB indexing `result`'s bytes, SelectStats); mode "protein" or "nucleotide"; free the subset before `result`"""
        if mode not in ("protein", "nucleotide"):
            raise ValueError("mode must be 'protein' or 'nucleotide'")
        cp = _SelectParams(0 if mode == "protein" else 1, 1 if only_extended else 0, int(min_contig_len))
        h = P(); st = SelectStats()
        _check(self.lib.plasship_select_contigs(self.h, result.h, source.h, cycles.h if cycles is not None else None, C.byref(cp), C.byref(h), C.byref(st)),
               "plasship_select_contigs")
        return SeqDB(self, h), st

    def write_fasta(self, db, path, cycles=None):
        """createhdb + convert2fasta of `db` into the file `path` (with a " cycle:<0|1>" field when `cycles` is given) -> FastaStats"""
        st = FastaStats()
        _check(self.lib.plasship_fasta_write(self.h, db.h, cycles.h if cycles is not None else None, os.fsencode(str(path)), C.byref(st)), "plasship_fasta_write")
        return st

    def write_subdb(self, db, path, cycles=None):
        """`createsubdb --subdb-mode 0` of a selection (data/nuclassemble.sh:170-176, 200-207): its entries gathered on the device and written
        as `path`, `path`.index, `path`.dbtype, plus `path`_cycle.index (the index lines of the keys in `cycles`) when `cycles` is given
        -> SubdbStats"""
        st = SubdbStats()
        _check(self.lib.plasship_subdb_write(self.h, db.h, cycles.h if cycles is not None else None, os.fsencode(str(path)), C.byref(st)), "plasship_subdb_write")
        return st

    def nuclassemble_db(self, db, path, num_iterations=8, k=22, min_seq_id=0.99, min_aln_len=0, max_seq_len=200000, chop_cycle=True,
                        only_extended=True, min_contig_len=1000):
        """`penguin nuclassemble --db-mode 1` on a resident nucleotide DB (data/nuclassemble.sh:95-207): the loop with cyclecheck after every
        iteration, RESULT = the rest + every circular contig, the `_only_assembled` and --min-contig-len selection against `db`, written with
        write_subdb -> (SelectStats, SubdbStats).  `db` stays the caller's."""
        km = KmermatchParams(k=k, kmer_per_seq_scale=0.1, include_only_extendable=True)
        rs = RescoreParams(min_seq_id=min_seq_id, min_aln_len=min_aln_len)
        asp = AssembleParams(min_seq_id=min_seq_id, max_seq_len=max_seq_len)
        cur, cyc_all = db, None
        for _ in range(num_iterations):
            c, _s = self.kmermatcher(cur, km)
            a, _s = self.rescorediagonal(cur, cur, c, rs)
            nxt, _s = self.assembleresults(cur, a, asp)
            a.free(); c.free()
            if cur is not db:
                cur.free()
            cyc, cur, cs = self.cyclecheck(nxt, max_seq_len=max_seq_len, chop_cycle=chop_cycle, with_rest=True)
            nxt.free()
            if cs.n_cyclic and cyc_all is None:
                cyc_all, cyc = cyc, None
            elif cs.n_cyclic:
                u = self.concatdbs(cyc_all, cyc, preserve_keys=True)
                cyc_all.free(); cyc_all = u
            if cyc is not None:
                cyc.free()
        result = self.concatdbs(cur, cyc_all, preserve_keys=True) if cyc_all is not None else cur
        sel, ss = self.select_contigs(result, db, "nucleotide", cycles=cyc_all, only_extended=only_extended, min_contig_len=min_contig_len)
        ds = self.write_subdb(sel, path, cycles=cyc_all)
        sel.free()
        if result is not cur:
            result.free()
        if cur is not db:
            cur.free()
        if cyc_all is not None:
            cyc_all.free()
        return ss, ds

    def guided_tail(self, nucl_result, nucl_source, reads, path, **nucl_par):
        """what `penguin guided_nuclassemble` does behind its guided loop, up to linclust (data/guidedNuclAssemble.sh:135-170): the extended
        ORFs of `nucl_result` (keys of `nucl_source` = nucl_6f_start_long whose entry grew, `$3 > $6`) concatenated with `reads`, then
        nuclassemble_db(merged, path, **nucl_par) -> (SelectStats, SubdbStats).  The three DBs stay the caller's."""
        only, _s = self.select_contigs(nucl_result, nucl_source, "nucleotide", only_extended=True, min_contig_len=0)
        merged = self.concatdbs(only, reads)
        only.free()
        try:
            return self.nuclassemble_db(merged, path, **nucl_par)
        finally:
            merged.free()

    def synth_read_pairs(self, par):
        """synthetic read pairs generated in HBM (include/plasship_synth.h) -> nucleotide read DB"""
        h = P(); st = SynthStats(); cp = par._c()
        _check(self.lib.plasship_synth_read_pairs(self.h, C.byref(cp), C.byref(h), C.byref(st)), "plasship_synth_read_pairs")
        return SeqDB(self, h), st

    # the library picks the variant from the DB type; this name mirrors the reference module for nucleotide DBs
    def nuclassembleresults(self, db, alns, par=None):
        if db.info()["dbtype"] != 1:
            raise ValueError("nuclassembleresults needs a nucleotide sequence DB")
        return self.assembleresults(db, alns, par or AssembleParams(min_seq_id=0.99, max_seq_len=200000))


class SeqDB:
    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h

    def info(self):
        n = C.c_size_t(); res = C.c_uint64(); mx = C.c_uint32(); ty = C.c_int(); nb = C.c_uint64()
        _check(self.ctx.lib.plasship_seqdb_info(self.h, C.byref(n), C.byref(res), C.byref(mx), C.byref(ty), C.byref(nb)), "plasship_seqdb_info")
        return dict(n=n.value, residues=res.value, max_entry_len=mx.value, dbtype=ty.value, data_bytes=nb.value)

    def write(self, path):
        _check(self.ctx.lib.plasship_seqdb_write(self.ctx.h, self.h, os.fsencode(path)), "plasship_seqdb_write")

    def digest(self):
        """(digest as 16 hex digits, entry bytes): order-independent digest of the resident DB (include/plasship.h: plasship_seqdb_digest)"""
        d = C.c_uint64(); b = C.c_uint64()
        _check(self.ctx.lib.plasship_seqdb_digest(self.ctx.h, self.h, C.byref(d), C.byref(b)), "plasship_seqdb_digest")
        return "%016x" % d.value, b.value

    def download(self):
        import numpy as np
        i = self.info()
        data = C.create_string_buffer(max(i["data_bytes"], 1))
        off = np.zeros(i["n"], dtype=np.uint64); elen = np.zeros(i["n"], dtype=np.uint32); key = np.zeros(i["n"], dtype=np.uint32)
        _check(self.ctx.lib.plasship_seqdb_download(self.ctx.h, self.h, data, off.ctypes.data, elen.ctypes.data, key.ctypes.data), "plasship_seqdb_download")
        return data.raw[:i["data_bytes"]], off, elen, key

    def free(self):
        if self.h:
            self.ctx.lib.plasship_seqdb_free(self.ctx.h, self.h); self.h = P()


class OrfHeaders:
    """header DB of an ORF DB (<db>_h), device resident"""
    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h

    def count(self):
        n = C.c_size_t()
        _check(self.ctx.lib.plasship_orfhdr_count(self.h, C.byref(n)), "plasship_orfhdr_count")
        return n.value

    def write(self, path):
        _check(self.ctx.lib.plasship_orfhdr_write(self.ctx.h, self.h, os.fsencode(path)), "plasship_orfhdr_write")

    def free(self):
        if self.h:
            self.ctx.lib.plasship_orfhdr_free(self.ctx.h, self.h); self.h = P()


class Candidates:
    def __init__(self, ctx, h, qdb, tdb):
        self.ctx, self.h, self.qdb, self.tdb = ctx, h, qdb, tdb

    def count(self):
        n = C.c_uint64(); r = C.c_int()
        _check(self.ctx.lib.plasship_cands_count(self.h, C.byref(n), C.byref(r)), "plasship_cands_count")
        return n.value

    def write(self, path):
        _check(self.ctx.lib.plasship_cands_write(self.ctx.h, self.h, self.qdb.h, os.fsencode(path)), "plasship_cands_write")

    def download(self):
        import numpy as np
        n = self.count()
        q = np.zeros(n, dtype=np.uint32); t = np.zeros(n, dtype=np.uint32); s = np.zeros(n, dtype=np.int32); d = np.zeros(n, dtype=np.uint16)
        _check(self.ctx.lib.plasship_cands_download(self.ctx.h, self.h, self.qdb.h, self.tdb.h, q.ctypes.data, t.ctypes.data, s.ctypes.data, d.ctypes.data), "plasship_cands_download")
        return q, t, s, d

    def free(self):
        if self.h:
            self.ctx.lib.plasship_cands_free(self.ctx.h, self.h); self.h = P()


class _PairList:
    """(representative, member) pairs over a DB, device resident; a subclass names the loader of the library with its entry points and their prefix"""
    def __init__(self, ctx, h, db):
        self.ctx, self.h, self.db = ctx, h, db      # keeps the DB alive (ids -> keys)

    def _call(self, name, *args):
        _check(getattr(self._load(), self._prefix + name)(*args), self._prefix + name)

    def count(self):
        """(members = DB size, clusters)"""
        n = C.c_uint64(); k = C.c_uint64()
        self._call("_count", self.h, C.byref(n), C.byref(k))
        return n.value, k.value

    def download(self, db=None):
        """(representative keys, member keys), sorted by representative key, then member key"""
        import numpy as np
        n = self.count()[0]
        rep = np.zeros(n, dtype=np.uint32); mem = np.zeros(n, dtype=np.uint32)
        self._call("_download", self.ctx.h, self.h, (db or self.db).h, rep.ctypes.data, mem.ctypes.data)
        return rep, mem

    def write(self, path, db=None):
        self._call("_write", self.ctx.h, self.h, (db or self.db).h, os.fsencode(path))

    def free(self):
        if self.h:
            getattr(self._load(), self._prefix + "_free")(self.ctx.h, self.h); self.h = P()


class Clusters(_PairList):
    """greedy clustering of a DB, device resident"""
    _load, _prefix = staticmethod(lambda: load_library().clust), "plasship_clusters"


class MergedClusters(_PairList):
    """what mergeclusters makes of two clusterings of a DB, device resident: the members in the merged DB's order"""
    _load, _prefix = staticmethod(load_linclust_library), "plasship_merged"

    def download(self):
        """(representative keys, member keys) in the merged DB's order"""
        return _PairList.download(self)

    def write(self, path):
        _PairList.write(self, path)


class Alignments:
    def __init__(self, ctx, h, qdb, tdb):
        self.ctx, self.h, self.qdb, self.tdb = ctx, h, qdb, tdb   # keeps the DBs alive (ids -> keys)

    def count(self):
        n = C.c_uint64()
        _check(self.ctx.lib.plasship_alns_count(self.h, C.byref(n)), "plasship_alns_count")
        return n.value

    def write(self, path):
        _check(self.ctx.lib.plasship_alns_write(self.ctx.h, self.h, os.fsencode(path)), "plasship_alns_write")

    def download(self):
        n = self.count()
        arr = (AlnRecord * max(n, 1))()
        _check(self.ctx.lib.plasship_alns_download(self.ctx.h, self.h, arr), "plasship_alns_download")
        return arr[:n]

    def free(self):
        if self.h:
            self.ctx.lib.plasship_alns_free(self.ctx.h, self.h); self.h = P()
