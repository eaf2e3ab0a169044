"""ctypes binding of libdnastore_amd.so (the C ABI of include/dnastore_amd.h).

There is no CPU fallback: if the shared library (host C++ + gfx950 HIP kernels) has not
been built, importing it raises, and device entry points fail with DNAS_E_DEVICE when no
GPU is present.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# DNAS_LIBRARY: another build of the same library (tools/run_asan.sh: the sanitizer build under dnastore_amd/asan/)
LIB_PATH = os.environ.get("DNAS_LIBRARY") or os.path.join(_HERE, "libdnastore_amd.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "dnastore_amd.h")

DNAS_OK = 0
READ_OK, READ_NO_PATH, READ_OUT_OVERFLOW, READ_TRACEBACK_FAIL = 0, 1, 2, 3
STRAND_FORWARD, STRAND_REVERSE, STRAND_BOTH = 0, 1, 2
ALIGN_FULL = -1
ALIGN_OK, ALIGN_NO_PATH, ALIGN_TOO_LARGE, ALIGN_TRACEBACK_FAIL = 0, 1, 2, 3
COUNTS_OK, COUNTS_NO_PATH, COUNTS_TOO_LARGE = 0, 1, 2
# planes of a pair's profile block, [6 + P, I + 1] ...
PROFILE_MATCH, PROFILE_DEL_OPEN, PROFILE_DEL_EXTEND, PROFILE_DUP = 0, 4, 5, 6
# ... and of the aggregate, [5 + P, n_positions]
PROFILE_SAME, PROFILE_TRANSITION, PROFILE_TRANSVERSION, PROFILE_SUM_DEL_OPEN, PROFILE_SUM_DEL_EXTEND, PROFILE_SUM_DUP = 0, 1, 2, 3, 4, 5
PROFILE_FROM_START, PROFILE_FROM_END = 0, 1
OP_MATCH, OP_DELETE, OP_DUP = 0, 1, 2
SCORE_VITERBI, SCORE_FORWARD = 0, 1
ASSIGN_OK, ASSIGN_NO_PATH, ASSIGN_NO_CANDIDATES = 0, 1, 2
CONSENSUS_OK, CONSENSUS_NO_PATH, CONSENSUS_NO_CANDIDATES, CONSENSUS_NO_READS = 0, 1, 2, 3
CLUSTER_OK, CLUSTER_NO_SKETCH, CLUSTER_EMPTY = 0, 1, 2
POLISH_OK, POLISH_NO_VOTERS, POLISH_NO_READS = 0, 1, 2
POLISH_MAX_INSERT = 4
TRIM_BOTH, TRIM_EITHER = 0, 1
TRIM_OK, TRIM_NO_ANCHOR, TRIM_TOO_SHORT = 0, 1, 2
TRIM_ANCHORS = {"both": TRIM_BOTH, "either": TRIM_EITHER}
SIM_OK, SIM_TOO_LARGE = 0, 1
RS_OK, RS_CORRECTED, RS_FAILED = 0, 1, 2
OUTER_OK, OUTER_DAMAGED, OUTER_NO_LENGTH, OUTER_BAD_LENGTH = 0, 1, 2, 3
STRAND_MODES = {"forward": STRAND_FORWARD, "reverse": STRAND_REVERSE, "both": STRAND_BOTH}
ERROR_NAMES = {-1: "DNAS_E_INVALID", -2: "DNAS_E_IO", -3: "DNAS_E_PARSE", -4: "DNAS_E_CYCLIC", -5: "DNAS_E_NOT_DNA",
               -6: "DNAS_E_BAD_BASE", -7: "DNAS_E_DEVICE", -8: "DNAS_E_NOMEM", -9: "DNAS_E_UNSUPPORTED"}


class DnasError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s: %s" % (ERROR_NAMES.get(code, code), msg))
        self.code = code


class MutatorParamsC(ctypes.Structure):
    _fields_ = [("p_del_open", ctypes.c_double), ("p_del_extend", ctypes.c_double), ("p_tan_dup", ctypes.c_double),
                ("p_transition", ctypes.c_double), ("p_transversion", ctypes.c_double),
                ("n_len", ctypes.c_int32), ("local", ctypes.c_int32), ("p_len", ctypes.c_double * 32)]


_I32P, _F64P, _U8P = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint8)


class FlatModelC(ctypes.Structure):
    _fields_ = [("n_states", ctypes.c_int32), ("max_dup_len", ctypes.c_int32), ("n_len", ctypes.c_int32),
                ("local", ctypes.c_int32), ("n_emit", ctypes.c_int32), ("n_null", ctypes.c_int32),
                ("ein_ptr", _I32P), ("ein_src", _I32P), ("ein_score", _F64P), ("ein_in", _U8P), ("ein_base", _U8P),
                ("nin_ptr", _I32P), ("nin_src", _I32P), ("nin_score", _F64P), ("nin_in", _U8P),
                ("eout_ptr", _I32P), ("eout_dst", _I32P), ("eout_score", _F64P),
                ("nout_ptr", _I32P), ("nout_dst", _I32P), ("nout_score", _F64P),
                ("mdl", _U8P), ("ctx", _U8P), ("topo", _I32P),
                ("no_gap", ctypes.c_double), ("del_open", ctypes.c_double), ("del_extend", ctypes.c_double),
                ("del_end", ctypes.c_double), ("tan_dup", ctypes.c_double), ("sub", ctypes.c_double * 16),
                ("len", _F64P), ("alphabet", ctypes.c_char * 64), ("sym_logp", ctypes.c_double * 128)]


class PairsViewC(ctypes.Structure):
    _fields_ = [("n_pairs", ctypes.c_int64), ("in_seqs", ctypes.c_void_p), ("in_off", ctypes.c_void_p),
                ("out_seqs", ctypes.c_void_p), ("out_off", ctypes.c_void_p), ("cm_in", ctypes.c_void_p),
                ("cm_in_off", ctypes.c_void_p), ("cm_out", ctypes.c_void_p), ("cm_out_off", ctypes.c_void_p)]


class FbStatsC(ctypes.Structure):
    _fields_ = [("kernel_ms", ctypes.c_double), ("pairs_onchip", ctypes.c_int64), ("pairs_streaming", ctypes.c_int64),
                ("lse_ops", ctypes.c_int64), ("out_nt", ctypes.c_int64), ("pairs_narrow", ctypes.c_int64)]


class BatchStatsC(ctypes.Structure):
    _fields_ = [("fill_ms", ctypes.c_double), ("traceback_ms", ctypes.c_double), ("fill_launches", ctypes.c_int64),
                ("columns", ctypes.c_int64), ("lattice_bytes", ctypes.c_int64), ("rounds", ctypes.c_int64),
                ("checkpointed_reads", ctypes.c_int64)]


class StrandStatsC(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int64) for k in ("reads", "reverse_won", "ties", "both_no_path", "tracebacks", "fill_columns",
                                              "pass2_columns")]


class ForwardStatsC(ctypes.Structure):
    _fields_ = [("score_ms", ctypes.c_double), ("items", ctypes.c_int64), ("cells", ctypes.c_int64), ("chunks", ctypes.c_int64)]


class CountsStatsC(ctypes.Structure):
    _fields_ = [("kernel_ms", ctypes.c_double)] + [(k, ctypes.c_int64) for k in ("cells", "chunks", "scratch_bytes",
                                                                                  "pairs_too_large", "waves")]


class AlignStatsC(ctypes.Structure):
    _fields_ = [("fill_ms", ctypes.c_double), ("traceback_ms", ctypes.c_double), ("cells", ctypes.c_int64),
                ("batches", ctypes.c_int64), ("pairs_too_large", ctypes.c_int64)]


class AssignStatsC(ctypes.Structure):
    _fields_ = [("score_ms", ctypes.c_double), ("fold_ms", ctypes.c_double), ("items", ctypes.c_int64),
                ("cells", ctypes.c_int64), ("chunks", ctypes.c_int64)]


class ConsensusStatsC(ctypes.Structure):
    _fields_ = [("score_ms", ctypes.c_double), ("fold_ms", ctypes.c_double), ("items", ctypes.c_int64), ("cells", ctypes.c_int64),
                ("chunks", ctypes.c_int64), ("candidates", ctypes.c_int64), ("encode_failures", ctypes.c_int64),
                ("decode_wall_ms", ctypes.c_double), ("candidates_wall_ms", ctypes.c_double), ("rescore_wall_ms", ctypes.c_double),
                ("polish_wall_ms", ctypes.c_double)]


class PolishStatsC(ctypes.Structure):
    _fields_ = ([("fill_ms", ctypes.c_double), ("vote_ms", ctypes.c_double)]
                + [(k, ctypes.c_int64) for k in ("rounds", "pairs", "cells", "batches", "lds_clusters", "hbm_clusters")])


class ClusterStatsC(ctypes.Structure):
    _fields_ = ([(k, ctypes.c_double) for k in ("sketch_ms", "filter_ms", "score_ms", "fold_ms")]
                + [(k, ctypes.c_int64) for k in ("pairs", "candidates", "items", "cells", "edges", "chunks", "clusters",
                                                 "strand_conflicts")])


class ClusterGateStatsC(ctypes.Structure):
    _fields_ = [("gate_ms", ctypes.c_double)] + [(k, ctypes.c_int64) for k in ("tested", "passed", "long_pairs", "word_steps")]


class TrimStatsC(ctypes.Structure):
    _fields_ = [("kernel_ms", ctypes.c_double)] + [(k, ctypes.c_int64) for k in ("items", "columns", "trimmed", "chunks", "devices")]


class SimulateStatsC(ctypes.Structure):
    _fields_ = ([("count_ms", ctypes.c_double), ("write_ms", ctypes.c_double)]
                + [(k, ctypes.c_int64) for k in ("batches", "bases_in", "bases_out", "ops", "reads_too_large", "devices")])


class RsStatsC(ctypes.Structure):
    _fields_ = [("kernel_ms", ctypes.c_double)] + [(k, ctypes.c_int64) for k in ("columns", "columns_solved", "launches", "devices")]


class OuterStatsC(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int64) for k in ("records", "dropped", "conflicts", "ties", "erased", "columns_ok", "columns_corrected",
                                              "columns_failed", "strands_fixed")] + [("rs", RsStatsC)]


def strand_mode(strands):
    """'forward' | 'reverse' | 'both' (or the DNAS_STRAND_* number) -> DNAS_STRAND_*."""
    if strands in STRAND_MODES:
        return STRAND_MODES[strands]
    if strands in (STRAND_FORWARD, STRAND_REVERSE, STRAND_BOTH) and not isinstance(strands, bool):
        return int(strands)
    raise ValueError("strands must be 'forward', 'reverse' or 'both', not %r" % (strands,))


SCORE_MODES = {"viterbi": SCORE_VITERBI, "forward": SCORE_FORWARD}


def score_mode(score):
    """'viterbi' | 'forward' (or the DNAS_SCORE_* number) -> DNAS_SCORE_*."""
    if score in SCORE_MODES:
        return SCORE_MODES[score]
    if score in (SCORE_VITERBI, SCORE_FORWARD) and not isinstance(score, bool):
        return int(score)
    raise ValueError("score must be 'viterbi' or 'forward', not %r" % (score,))


def declared_symbols():
    """Every function name include/dnastore_amd.h declares."""
    text = open(HEADER_PATH).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dnas_[a-z0-9_]+)\s*\(", text)))


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s is missing: build it with `make -C dnastore_amd/csrc` "
                          "(or __graft_entry__.build()); there is no CPU fallback" % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    vp, cp, i64, sz = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int64, ctypes.c_size_t
    P = ctypes.POINTER
    sigs = {
        "dnas_machine_load_json": (ctypes.c_int, [cp, P(vp)]),
        "dnas_machine_parse_json": (ctypes.c_int, [cp, sz, P(vp)]),
        "dnas_machine_free": (None, [vp]),
        "dnas_machine_n_states": (ctypes.c_int32, [vp]),
        "dnas_machine_write_json": (ctypes.c_int, [vp, P(vp), P(sz)]),
        "dnas_machine_compose": (ctypes.c_int, [vp, vp, P(vp)]),
        "dnas_decode_exact": (ctypes.c_int, [vp, cp, sz, P(vp), P(sz)]),
        "dnas_symbols_to_bytes": (ctypes.c_int, [cp, sz, P(vp), P(sz)]),
        "dnas_encode_symbols": (ctypes.c_int, [vp, cp, sz, P(vp), P(sz)]),
        "dnas_encode_bytes": (ctypes.c_int, [vp, cp, sz, P(vp), P(sz)]),
        "dnas_mutator_params_from_flags": (ctypes.c_int, [ctypes.c_double] * 5 + [ctypes.c_int, ctypes.c_int, P(MutatorParamsC)]),
        "dnas_mutator_params_load_json": (ctypes.c_int, [cp, P(MutatorParamsC)]),
        "dnas_flatten": (ctypes.c_int, [vp, P(MutatorParamsC), P(vp)]),
        "dnas_flat_view": (P(FlatModelC), [vp]),
        "dnas_flat_free": (None, [vp]),
        "dnas_model_create": (ctypes.c_int, [P(FlatModelC), ctypes.c_int, sz, P(vp)]),
        "dnas_model_create_ex": (ctypes.c_int, [P(FlatModelC), ctypes.c_int, sz, cp, P(vp)]),
        "dnas_model_destroy": (None, [vp]),
        "dnas_viterbi_batch": (ctypes.c_int, [vp, i64, vp, vp, vp, vp, vp, vp, vp]),
        "dnas_viterbi_batch_device": (ctypes.c_int, [vp, i64, vp, vp, vp, vp, vp, vp, vp]),
        "dnas_viterbi_batch_strands": (ctypes.c_int, [vp, i64, vp, vp, ctypes.c_int, vp, vp, vp, vp, vp, vp]),
        "dnas_viterbi_batch_strands_device": (ctypes.c_int, [vp, i64, vp, vp, ctypes.c_int, vp, vp, vp, vp, vp, vp]),
        "dnas_slot_needed": (ctypes.c_uint64, [vp, ctypes.c_uint64]),
        "dnas_reverse_complement": (ctypes.c_int, [vp, sz, vp]),
        "dnas_model_last_strand_stats": (ctypes.c_int, [vp, P(StrandStatsC)]),
        "dnas_decode_fastseqs_strands": (ctypes.c_int, [cp, vp, P(MutatorParamsC), ctypes.c_int, ctypes.c_int, ctypes.c_int, P(vp)]),
        "dnas_decoded_strand": (ctypes.c_int, [vp, i64]),
        "dnas_model_sync": (ctypes.c_int, [vp]),
        "dnas_model_tier": (cp, [vp]),
        "dnas_tiera_plan_slots": (ctypes.c_int, [P(FlatModelC), vp, vp, vp, vp]),
        "dnas_tiera_plan_tables": (ctypes.c_int, [P(FlatModelC), vp, vp, ctypes.c_size_t, vp, vp, vp]),
        "dnas_model_debug_words": (ctypes.c_int, [vp, vp]),
        "dnas_tiera_precompile": (ctypes.c_int, [P(FlatModelC), ctypes.c_char_p, sz]),
        "dnas_tierc_precompile": (ctypes.c_int, [P(FlatModelC), ctypes.c_int32, ctypes.c_char_p, sz]),
        "dnas_tierc_plan": (ctypes.c_int, [P(FlatModelC), ctypes.c_int32, vp, vp, vp, sz, vp, vp, vp, vp, vp]),
        "dnas_tierc_plan_proxies": (ctypes.c_int, [P(FlatModelC), ctypes.c_int32, vp, vp, sz]),
        "dnas_model_cluster_census": (ctypes.c_int, [vp, vp, vp]),
        "dnas_tune_record_name": (ctypes.c_int, [vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_char_p, ctypes.c_size_t]),
        "dnas_kernel_source_hash": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t]),
        "dnas_model_last_stats": (ctypes.c_int, [vp, P(BatchStatsC)]),
        "dnas_model_last_arena_slices": (ctypes.c_int, [vp, P(ctypes.c_int64)]),
        "dnas_model_read_lattice": (ctypes.c_int, [vp, i64, i64, vp]),
        "dnas_fwdback_estep": (ctypes.c_int, [P(MutatorParamsC), ctypes.c_int, i64] + [vp] * 8 + [ctypes.c_int, vp, vp, vp]),
        "dnas_fb_create": (ctypes.c_int, [ctypes.c_int, P(vp)]),
        "dnas_fb_load_pairs": (ctypes.c_int, [vp, i64] + [vp] * 8),
        "dnas_fb_estep": (ctypes.c_int, [vp, P(MutatorParamsC), ctypes.c_int, vp, vp, vp]),
        "dnas_fb_last_stats": (ctypes.c_int, [vp, P(FbStatsC)]),
        "dnas_fb_devices": (ctypes.c_int, [vp]),
        "dnas_fb_destroy": (None, [vp]),
        "dnas_baum_welch": (ctypes.c_int, [P(MutatorParamsC), ctypes.c_int, i64] + [vp] * 8 + [ctypes.c_int, P(MutatorParamsC), vp]),
        "dnas_stockholm_read": (ctypes.c_int, [cp, P(vp)]),
        "dnas_mutator_scores": (ctypes.c_int, [P(MutatorParamsC), vp]),
        "dnas_align_pairs": (ctypes.c_int, [P(MutatorParamsC), ctypes.c_int32, i64, vp, vp, vp, vp, ctypes.c_int, sz,
                                            vp, vp, vp, vp, vp, P(AlignStatsC)]),
        "dnas_align_pairs_host": (ctypes.c_int, [P(MutatorParamsC), ctypes.c_int32, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "dnas_pair_likelihoods": (ctypes.c_int, [P(MutatorParamsC), ctypes.c_int32, i64, vp, vp, vp, vp, vp, ctypes.c_int, vp,
                                                 P(ForwardStatsC)]),
        "dnas_pair_likelihoods_host": (ctypes.c_int, [P(MutatorParamsC), ctypes.c_int32, i64, vp, vp, vp, vp, vp, ctypes.c_int, vp]),
        "dnas_pair_counts": (ctypes.c_int, [P(MutatorParamsC), ctypes.c_int32, i64, vp, vp, vp, vp, vp, ctypes.c_int, sz,
                                            vp, vp, vp, vp, vp, vp, P(CountsStatsC)]),
        "dnas_pair_counts_host": (ctypes.c_int, [P(MutatorParamsC), ctypes.c_int32, i64, vp, vp, vp, vp, vp, ctypes.c_int,
                                                 vp, vp, vp, vp, vp, vp]),
        "dnas_pair_profiles": (ctypes.c_int, [P(MutatorParamsC), ctypes.c_int32, i64, vp, vp, vp, vp, vp, ctypes.c_int, sz,
                                              ctypes.c_int32, i64, vp, vp, vp, vp, vp, P(CountsStatsC)]),
        "dnas_pair_profiles_host": (ctypes.c_int, [P(MutatorParamsC), ctypes.c_int32, i64, vp, vp, vp, vp, vp, ctypes.c_int,
                                                   ctypes.c_int32, i64, vp, vp, vp, vp, vp]),
        "dnas_baum_welch_pairs": (ctypes.c_int, [P(MutatorParamsC), ctypes.c_int32, i64, vp, vp, vp, vp, vp, ctypes.c_int, sz,
                                                 ctypes.c_int32, P(MutatorParamsC), vp, vp, vp, vp]),
        "dnas_baum_welch_pairs_host": (ctypes.c_int, [P(MutatorParamsC), ctypes.c_int32, i64, vp, vp, vp, vp, vp, ctypes.c_int,
                                                      ctypes.c_int32, P(MutatorParamsC), vp, vp, vp, vp]),
        "dnas_assigner_create": (ctypes.c_int, [P(MutatorParamsC), ctypes.c_int32, i64, vp, vp, ctypes.c_int, P(vp)]),
        "dnas_assigner_run": (ctypes.c_int, [vp, i64, vp, vp, ctypes.c_int, vp, vp, vp, vp, vp, vp, vp, vp, P(AssignStatsC)]),
        "dnas_assigner_destroy": (None, [vp]),
        "dnas_assign_reads": (ctypes.c_int, [P(MutatorParamsC), ctypes.c_int32, i64, vp, vp, i64, vp, vp, ctypes.c_int, vp, vp,
                                             ctypes.c_int, vp, vp, vp, vp, vp, vp, P(AssignStatsC)]),
        "dnas_assign_reads_host": (ctypes.c_int, [P(MutatorParamsC), ctypes.c_int32, i64, vp, vp, i64, vp, vp, ctypes.c_int, vp, vp,
                                                  vp, vp, vp, vp, vp, vp]),
        "dnas_consensus_score": (ctypes.c_int, [P(MutatorParamsC), ctypes.c_int32, i64, i64, vp, vp, vp, i64, vp, vp, vp, vp, ctypes.c_int,
                                                vp, vp, vp, vp, vp, P(ConsensusStatsC)]),
        "dnas_consensus_score_host": (ctypes.c_int, [P(MutatorParamsC), ctypes.c_int32, i64, i64, vp, vp, vp, i64, vp, vp, vp, vp,
                                                     vp, vp, vp, vp, vp]),
        "dnas_consensus_score_ex": (ctypes.c_int, [P(MutatorParamsC), ctypes.c_int32, i64, i64, vp, vp, vp, i64, vp, vp, vp, vp, ctypes.c_int,
                                                   ctypes.c_int, vp, vp, vp, vp, vp, vp, P(ConsensusStatsC)]),
        "dnas_consensus_score_host_ex": (ctypes.c_int, [P(MutatorParamsC), ctypes.c_int32, i64, i64, vp, vp, vp, i64, vp, vp, vp, vp,
                                                        ctypes.c_int, vp, vp, vp, vp, vp, vp]),
        "dnas_viterbi_clusters_scored": (ctypes.c_int, [vp, vp, P(MutatorParamsC), ctypes.c_int32, i64, vp, vp, vp, i64, ctypes.c_int,
                                                        ctypes.c_int32] + [vp] * 13 + [P(vp)] + [vp] * 6
                                         + [ctypes.c_int, vp, P(ConsensusStatsC)]),
        "dnas_viterbi_clusters": (ctypes.c_int, [vp, vp, P(MutatorParamsC), ctypes.c_int32, i64, vp, vp, vp, i64, ctypes.c_int] + [vp] * 12
                                  + [P(ConsensusStatsC)]),
        "dnas_viterbi_clusters_ex": (ctypes.c_int, [vp, vp, P(MutatorParamsC), ctypes.c_int32, i64, vp, vp, vp, i64, ctypes.c_int, ctypes.c_int32]
                                     + [vp] * 13 + [P(vp)] + [vp] * 6 + [P(ConsensusStatsC)]),
        "dnas_model_device": (ctypes.c_int, [vp]),
        "dnas_cluster_consensus": (ctypes.c_int, [P(MutatorParamsC), ctypes.c_int32, i64, vp, vp, i64, vp, vp, vp, vp, ctypes.c_int32,
                                                  ctypes.c_int, sz, P(vp), vp, vp, vp, vp, vp, P(PolishStatsC)]),
        "dnas_cluster_consensus_host": (ctypes.c_int, [P(MutatorParamsC), ctypes.c_int32, i64, vp, vp, i64, vp, vp, vp, vp, ctypes.c_int32,
                                                       P(vp), vp, vp, vp, vp, vp]),
        "dnas_cluster_reads": (ctypes.c_int, [P(MutatorParamsC), ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                              ctypes.c_double, i64, vp, vp, ctypes.c_int, vp, vp, vp, vp, P(vp), P(vp), P(vp), P(i64),
                                              P(ClusterStatsC)]),
        "dnas_cluster_reads_host": (ctypes.c_int, [P(MutatorParamsC), ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                                   ctypes.c_double, i64, vp, vp, vp, vp, vp, vp, P(vp), P(vp), P(vp), P(i64),
                                                   P(ClusterStatsC)]),
        "dnas_cluster_reads_gated": (ctypes.c_int, [P(MutatorParamsC), ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                                    ctypes.c_double, ctypes.c_int32, i64, vp, vp, ctypes.c_int, vp, vp, vp, vp, P(vp), P(vp),
                                                    P(vp), P(i64), P(ClusterStatsC), P(ClusterGateStatsC)]),
        "dnas_cluster_reads_gated_host": (ctypes.c_int, [P(MutatorParamsC), ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                                         ctypes.c_double, ctypes.c_int32, i64, vp, vp, vp, vp, vp, vp, P(vp), P(vp), P(vp),
                                                         P(i64), P(ClusterStatsC), P(ClusterGateStatsC)]),
        "dnas_clusterer_create": (ctypes.c_int, [P(MutatorParamsC), ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                                 ctypes.c_double, ctypes.c_int32, ctypes.c_int, P(vp)]),
        "dnas_clusterer_add": (ctypes.c_int, [vp, i64, vp, vp, P(ClusterStatsC), P(ClusterGateStatsC)]),
        "dnas_clusterer_reads": (i64, [vp]),
        "dnas_clusterer_result": (ctypes.c_int, [vp, vp, vp, vp, vp, P(vp), P(vp), P(vp), P(i64), P(ClusterStatsC),
                                                 P(ClusterGateStatsC)]),
        "dnas_clusterer_destroy": (None, [vp]),
        "dnas_edit_distances": (ctypes.c_int, [i64, vp, i64, vp, vp, ctypes.c_int, vp]),
        "dnas_edit_distances_host": (ctypes.c_int, [i64, vp, i64, vp, vp, vp]),
        "dnas_trim_reads": (ctypes.c_int, [i64, vp, vp, i64, vp, vp] + [ctypes.c_int32] * 4 + [ctypes.c_int] + [vp] * 7 + [P(TrimStatsC)]),
        "dnas_trim_reads_host": (ctypes.c_int, [i64, vp, vp, i64, vp, vp] + [ctypes.c_int32] * 4 + [vp] * 7),
        "dnas_simulate_reads": (ctypes.c_int, [P(MutatorParamsC), i64, vp, vp, i64, vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_double,
                                               ctypes.c_int, ctypes.c_int, sz, P(vp), P(vp), P(vp), P(vp), P(vp), vp, P(SimulateStatsC)]),
        "dnas_simulate_reads_host": (ctypes.c_int, [P(MutatorParamsC), i64, vp, vp, i64, vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_double,
                                                    ctypes.c_int, P(vp), P(vp), P(vp), P(vp), P(vp), vp]),
        "dnas_simulate_draw_bits": (ctypes.c_uint64, [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32]),
        "dnas_rs_encode": (ctypes.c_int, [ctypes.c_int32] * 3 + [i64, vp, vp, P(RsStatsC), ctypes.c_int]),
        "dnas_rs_decode": (ctypes.c_int, [ctypes.c_int32] * 3 + [i64] + [vp] * 6 + [P(RsStatsC), ctypes.c_int]),
        "dnas_rs_encode_host": (ctypes.c_int, [ctypes.c_int32] * 3 + [i64, vp, vp]),
        "dnas_rs_decode_host": (ctypes.c_int, [ctypes.c_int32] * 3 + [i64] + [vp] * 6),
        "dnas_outer_blocks": (i64, [i64, ctypes.c_int32, ctypes.c_int32]),
        "dnas_outer_crc8": (ctypes.c_uint8, [vp, i64]),
        "dnas_outer_frame": (ctypes.c_int, [i64, vp, ctypes.c_int32, vp]),
        "dnas_outer_encode": (ctypes.c_int, [vp, i64] + [ctypes.c_int32] * 3 + [ctypes.c_int, ctypes.c_int, P(i64), P(vp)]),
        "dnas_outer_decode": (ctypes.c_int, [i64, vp, vp, vp] + [ctypes.c_int32] * 3 + [i64, ctypes.c_int, ctypes.c_int, P(vp), P(i64),
                                                P(ctypes.c_int32), vp, vp, vp, P(vp), P(i64), P(OuterStatsC)]),
        "dnas_cluster_sketch_host": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, i64, vp, vp, vp]),
        "dnas_cluster_candidates_host": (ctypes.c_int, [P(MutatorParamsC), ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                                        i64, vp, vp, P(vp), P(vp), P(i64)]),
        "dnas_alignment_expand": (ctypes.c_int, [ctypes.c_int32, vp, i64, vp, i64, vp, i64, vp, vp, vp, vp, vp]),
        "dnas_stockholm_write": (ctypes.c_int, [i64, P(cp), P(cp), P(cp), P(cp), P(vp), P(sz)]),
        "dnas_pairs_get": (P(PairsViewC), [vp]),
        "dnas_pairs_free": (None, [vp]),
        "dnas_mutator_params_json": (ctypes.c_int, [P(MutatorParamsC), ctypes.c_char_p, sz]),
        "dnas_mutator_counts_json": (ctypes.c_int, [vp, ctypes.c_int32, ctypes.c_char_p, sz]),
        "dnas_decode_fastseqs": (ctypes.c_int, [cp, vp, P(MutatorParamsC), ctypes.c_int, P(vp)]),
        "dnas_decode_fastseqs_ex": (ctypes.c_int, [cp, vp, P(MutatorParamsC), ctypes.c_int, ctypes.c_int, P(vp)]),
        "dnas_decoded_tier": (cp, [vp]),
        "dnas_decoded_devices": (ctypes.c_int, [vp]),
        "dnas_decoded_events": (i64, [vp, i64, P(vp)]),
        "dnas_device_count": (ctypes.c_int, []),
        "dnas_model_set_event_log": (ctypes.c_int, [vp, ctypes.c_int]),
        "dnas_model_read_events": (ctypes.c_int, [vp, i64, vp, i64, vp]),
        "dnas_decoded_count": (i64, [vp]),
        "dnas_decoded_name": (cp, [vp, i64]),
        "dnas_decoded_seq": (cp, [vp, i64]),
        "dnas_decoded_loglike": (ctypes.c_double, [vp, i64]),
        "dnas_decoded_free": (None, [vp]),
        "dnas_fastseqs_read": (ctypes.c_int, [cp, P(vp)]),
        "dnas_fastseqs_count": (i64, [vp]),
        "dnas_fastseqs_name": (cp, [vp, i64]),
        "dnas_fastseqs_seq": (cp, [vp, i64]),
        "dnas_fastseqs_free": (None, [vp]),
        "dnas_last_error": (cp, []),
        "dnas_free": (None, [vp]),
        "dnas_has_device_code": (ctypes.c_int, []),
        "dnas_debug_alloc_stats": (ctypes.c_int, [P(ctypes.c_int64), ctypes.c_int]),
    }
    for name, (res, args) in sigs.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def check(rc):
    if rc != DNAS_OK:
        raise DnasError(rc, lib().dnas_last_error().decode(errors="replace"))
