"""ctypes binding of libsdpcut_hip.so (C-ABI declared in include/sdpcut.h).

This is the only place where the host code touches native code, mirroring how the
reference reaches NNs.so through ctypes (cut_select_qp.py:284-303).  There is no CPU
fallback: a missing library or a missing gfx950 device raises.
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SDPCUT_LIB") or os.path.join(HERE, "libsdpcut_hip.so")   # env: experiment builds
# the reference's own FFI (six symbols of NNs.so) lives in a sibling library that binds to the one above privately
NNS_LIB_PATH = os.path.join(HERE, "libsdpcut_nns.so")

EIG, NN = 1, 2
SDP = 4                  # exact optimum of the small SDP the MLP estimates (sdpcut_score, include/sdpcut.h)
STRAT_FEAS, STRAT_OPT, STRAT_COMB = 1, 2, 4
STRAT_EXACT = 3          # strategy 2 on the exact measure; accepted only with OPT_EXACT_SDP
EFF = 8                  # efficacy of the cut row a round would emit, its objective parallelism and their score (sdpcut_score, include/sdpcut.h)
STRAT_EFF = 6            # strategy 2's ranking on the efficacy score
PART_STRONG = 104
PART_COMBALL = 105
KERNEL_MFMA, KERNEL_SIMPLE, KERNEL_VALU = 0, 1, 2
OPT_KERNEL, OPT_TIMING, OPT_FUSE_KEYS, OPT_AUTO_REGIME, OPT_FUSED_TAIL, OPT_COOP_LAUNCH, OPT_EIG_KERNEL, OPT_STREAM_PRIORITY, OPT_SIDE_STREAMS, OPT_ONE_LAUNCH, OPT_PREFILTER = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11
OPT_EXACT_HEAD = 12      # NN-ranked heads ordered and reported by reference-order obj_improve (include/sdpcut.h)
STAT_ROUNDS, STAT_SELECT_FALLBACKS, STAT_SCORED, STAT_TIE_SPLITS, STAT_DIRECT_SELECTIONS, STAT_PF_BIN, STAT_PF_FLOOR, STAT_PF_COUNT = 1, 2, 3, 4, 5, 6, 7, 8
STAT_EXACT_HEAD, STAT_EXACT_GAVE_UP, STAT_EXACT_RETRIES = 9, 10, 11
OPT_EXACT_SDP = 13       # strategy 3 accepted by the ranking and round calls (include/sdpcut.h)
OPT_COUNT_RANK = 14      # the sort tail of a selection ranks by counting in one launch (include/sdpcut.h); default on
STAT_SDP_UNCONVERGED = 12
OPT_SKIP_NONVIOLATED = 15   # fused combined rounds run the MLP for violated candidates only (include/sdpcut.h); 0 never, 1 long lists (default), 2 every list
STAT_NN_SKIPPED, STAT_NN_COMPLETIONS = 14, 15   # candidates the last such launch skipped; NN launches that completed a partial measure
OPT_FP32_FILTER = 16     # the skipping launch filters the violated candidates in fp32 ahead of the fp64 pass (include/sdpcut.h); default on
STAT_NN_EVALUATED = 16   # fp64 MLP evaluations of the last scoring launch that ran the network
STAT_POINTS_REDONE = 13   # points of batched rounds served by the single-point round inside the call (include/sdpcut.h)
STAT_TRI_POINTS_FAST = 19   # points of tri_round_csr_points answered by its one-wait route (include/sdpcut.h)
STAT_DIVERSE_POINTS_FAST = 17   # points of round_csr_points_diverse answered by its one-wait route (include/sdpcut.h)
OPT_INJECT_GIVEUP = 17   # TEST ONLY: the bounded device waits give up unasked (include/sdpcut.h); value = inject_giveup(site, first, count)
STAT_INJECTED = 18       # TEST ONLY: launches the option has hit
OPT_EMIT_HEAD = 18       # the skipping score launch emits its strong members, the strong regime selects from that list (include/sdpcut.h); default on
OPT_EMIT_CAP = 19        # TEST ONLY: capacity of that list in entries (0: what the workspace gives)
STAT_EMITTED_SELECTIONS = 20   # selections whose head came from the emitted list
STAT_NODE_EVAL_POINTS = 21     # points evaluated by node_eval_points since the handle was made
INJECT_SELECT, INJECT_LOOKBACK = 1, 2


def inject_giveup(site, first=0, count=1):
    """SDPCUT_INJECT_GIVEUP(site, first, count) of include/sdpcut.h: the value of OPT_INJECT_GIVEUP."""
    if site not in (INJECT_SELECT, INJECT_LOOKBACK) or not 0 <= first <= 255 or not 1 <= count <= 255:
        raise ValueError("inject_giveup: site 1..2, first 0..255, count 1..255")
    return (site << 16) | (first << 8) | count


BATCH_MAX_POINTS = 256   # SDPCUT_BATCH_MAX_POINTS: most LP points of one score_points / round_csr_points call
DIVERSE_MAX_POOL = 16384   # SDPCUT_DIVERSE_MAX_POOL: longest pool of round_csr_diverse / list of filter_parallel
MULTI_MAX_PER_SET = 5      # SDPCUT_MULTI_MAX_PER_SET: most eigen-cuts one index set offers (round_csr_multi / cut_rows_all)
POOL_MAX_ROWS = 4194304    # SDPCUT_POOL_MAX_ROWS: largest capacity of a cut pool (pool_create)
ROW_LD = 20
POOL_SEP_LP, POOL_SEP_PARKED = 1, 2     # SDPCUT_POOL_SEP_*: the rows pool_separate_points examines, by state
POOL_SEP_MAX_RETURN = 4096              # SDPCUT_POOL_SEP_MAX_RETURN: most rows a point gets back from pool_separate_points
POOL_SEP_MAX_BLOCK_BYTES = 256 << 20    # largest result block of one pool_separate_points call (csrc/pool_points_layout.h)

_c = ctypes
_i32p = _c.POINTER(_c.c_int32)
_i64p = _c.POINTER(_c.c_int64)
_dp = _c.POINTER(_c.c_double)
_vp = _c.c_void_p

class RoundCsr(_c.Structure):
    """sdpcut_round_csr_t of include/sdpcut.h"""
    _fields_ = [("cap", _c.c_int64), ("n_out", _c.c_int64), ("n_total", _c.c_int64), ("new_strat", _c.c_int32), ("row_ld", _c.c_int32),
                ("counters", _c.c_int64 * 4), ("idx", _vp), ("score", _vp), ("lam_min", _vp), ("ks", _vp), ("set_inds", _vp),
                ("n_rows", _c.c_int64), ("nnz", _c.c_int64), ("row_entry", _vp), ("indptr", _vp), ("indices", _vp),
                ("values", _vp), ("rhs", _vp)]

# the same record as a numpy dtype: the P records of a batched round are read as one structured array
_ROUND_CSR_DTYPE = np.dtype([("cap", "<i8"), ("n_out", "<i8"), ("n_total", "<i8"), ("new_strat", "<i4"), ("row_ld", "<i4"), ("counters", "<i8", (4,)),
                             ("idx", "<u8"), ("score", "<u8"), ("lam_min", "<u8"), ("ks", "<u8"), ("set_inds", "<u8"), ("n_rows", "<i8"),
                             ("nnz", "<i8"), ("row_entry", "<u8"), ("indptr", "<u8"), ("indices", "<u8"), ("values", "<u8"), ("rhs", "<u8")])
assert _ROUND_CSR_DTYPE.itemsize == _c.sizeof(RoundCsr)


class TriCsr(_c.Structure):
    """sdpcut_tri_csr_t of include/sdpcut.h"""
    _fields_ = [("cap", _c.c_int64), ("n_rows", _c.c_int64), ("n_violated", _c.c_int64), ("nnz", _c.c_int64), ("entry", _vp), ("viol", _vp),
                ("indptr", _vp), ("indices", _vp), ("values", _vp), ("rhs", _vp)]


class RoundMulti(_c.Structure):
    """sdpcut_round_multi_t of include/sdpcut.h"""
    _fields_ = [("csr", RoundCsr), ("row_cap", _c.c_int64), ("n_used", _c.c_int64), ("quota_hit", _c.c_int32), ("reserved", _c.c_int32),
                ("n_neg", _vp), ("row_lam", _vp), ("row_rank", _vp)]


class DiverseInfo(_c.Structure):
    """sdpcut_diverse_info_t of include/sdpcut.h"""
    _fields_ = [("pool", _c.c_int64), ("examined", _c.c_int64), ("skipped_nonviolated", _c.c_int64), ("rejected_parallel", _c.c_int64)]


class PoolParams(_c.Structure):
    """sdpcut_pool_params_t of include/sdpcut.h"""
    _fields_ = [("tight_tol", _c.c_double), ("viol_tol", _c.c_double), ("max_age", _c.c_int32), ("drop_age", _c.c_int32),
                ("max_return", _c.c_int64)]


class PoolStep(_c.Structure):
    """sdpcut_pool_step_t of include/sdpcut.h"""
    _fields_ = [("n_in_lp", _c.c_int64), ("n_parked", _c.c_int64), ("n_violated", _c.c_int64), ("n_dropped", _c.c_int64),
                ("n_leave", _c.c_int64), ("n_enter", _c.c_int64), ("enter_nnz", _c.c_int64), ("leave", _vp), ("enter", _vp),
                ("dropped", _vp), ("enter_indptr", _vp), ("enter_indices", _vp), ("enter_values", _vp), ("enter_rhs", _vp),
                ("enter_sense", _vp), ("enter_key", _vp)]


class PoolSep(_c.Structure):
    """sdpcut_pool_sep_t of include/sdpcut.h"""
    _fields_ = [("n_violated", _c.c_int64), ("n_rows", _c.c_int64), ("nnz", _c.c_int64), ("select_passes", _c.c_int32),
                ("serial", _vp), ("key", _vp), ("indptr", _vp), ("indices", _vp), ("values", _vp), ("rhs", _vp), ("sense", _vp)]


class NodeEval(_c.Structure):
    """sdpcut_node_eval_t of include/sdpcut.h"""
    _fields_ = [("f_point", _c.c_double), ("f_local", _c.c_double), ("branch_score", _c.c_double), ("branch_val", _c.c_double),
                ("sweeps", _c.c_int32), ("moves", _c.c_int32), ("branch_var", _c.c_int32), ("reserved", _c.c_int32), ("x_local", _vp)]


class DenseRound(_c.Structure):
    """sdpcut_dense_round_t of include/sdpcut.h"""
    _fields_ = [("dim", _c.c_int32), ("n_rows", _c.c_int32), ("sweeps", _c.c_int32), ("reserved", _c.c_int32), ("row_len", _c.c_int64),
                ("eigvals", _vp), ("cols", _vp), ("values", _vp), ("rhs", _vp)]


# name -> argtypes (restype is c_int unless listed in _RESTYPES); kept in one table so that the
# CPU test-suite can check that the library exports every symbol the header declares
SIGNATURES = {
    "sdpcut_version": [],
    "sdpcut_last_error": [_vp],
    "sdpcut_create": [_c.c_int, _c.POINTER(_vp)],
    "sdpcut_destroy": [_vp],
    "sdpcut_set_option": [_vp, _c.c_int, _c.c_int64],
    "sdpcut_set_stream": [_vp, _vp],
    "sdpcut_get_stat": [_vp, _c.c_int, _i64p],
    "sdpcut_get_filter_margin": [_vp, _c.c_int, _dp],
    "sdpcut_filter_audit": [_vp, _dp],
    "sdpcut_filter_audit_margins": [_vp, _dp, _dp],
    "sdpcut_synchronize": [_vp],
    "sdpcut_wake": [_vp],
    "sdpcut_set_network": [_vp, _c.c_int, _c.c_int, _i32p, _dp, _c.c_int64],
    "sdpcut_set_instance": [_vp, _c.c_int32, _dp],
    "sdpcut_set_candidates": [_vp, _c.c_int64, _i32p, _c.c_int32, _i32p, _c.c_int64],
    "sdpcut_set_candidates_philox": [_vp, _c.c_int32, _c.c_int64, _c.c_uint64, _c.c_int64],
    "sdpcut_set_candidates_cover": [_vp, _c.POINTER(_c.c_uint8), _c.c_int32, _c.c_int64, _i64p],
    "sdpcut_set_candidates_cover_ch": [_vp, _c.POINTER(_c.c_uint8), _c.POINTER(_c.c_uint8), _c.c_int32, _c.c_int32, _c.c_int64, _i64p],
    "sdpcut_set_candidates_cover_split": [_vp, _vp, _c.POINTER(_c.c_uint8), _c.POINTER(_c.c_uint8), _c.c_int32, _i64p, _i64p],
    "sdpcut_get_candidates": [_vp, _c.c_int64, _i64p, _i32p, _i32p],
    "sdpcut_set_builtin_networks": [_vp, _c.c_int],
    "sdpcut_set_point": [_vp, _dp],
    "sdpcut_point_buffer": [_vp, _c.POINTER(_dp)],
    "sdpcut_set_point_device": [_vp, _vp],
    "sdpcut_set_box": [_vp, _dp, _dp],
    "sdpcut_get_box": [_vp, _dp, _dp, _c.POINTER(_c.c_int)],
    "sdpcut_get_box_tables": [_vp, _dp, _dp],
    "sdpcut_score": [_vp, _c.c_uint32],
    "sdpcut_get_scores": [_vp, _dp, _dp],
    "sdpcut_get_sdp_scores": [_vp, _dp, _dp],
    "sdpcut_set_objective": [_vp, _c.c_int64, _dp],
    "sdpcut_set_efficacy_weight": [_vp, _c.c_double],
    "sdpcut_get_efficacy": [_vp, _dp, _dp, _dp],
    "sdpcut_rank": [_vp, _c.c_int, _c.c_int64, _c.c_int64, _i64p, _dp, _i64p, _i32p, _i64p],
    "sdpcut_rank_device": [_vp, _c.c_int, _c.c_int64, _c.c_int64, _vp, _vp, _i64p, _i64p, _i32p, _i64p],
    "sdpcut_rank_fetch": [_vp, _c.c_int64, _c.c_int64, _i64p, _dp],
    "sdpcut_merge_topk_device": [_vp, _c.c_int64, _vp, _vp, _vp, _c.c_int64, _vp, _vp],
    "sdpcut_gather_scores_device": [_vp, _c.c_int64, _vp, _vp, _vp],
    "sdpcut_cut_rows": [_vp, _c.c_int64, _i64p, _dp, _dp, _dp, _i64p, _i32p],
    "sdpcut_select_round": [_vp, _c.c_int, _c.c_int64, _c.c_int32, _i64p, _dp, _dp, _dp, _dp, _i32p, _i64p, _i64p, _i32p, _i64p],
    "sdpcut_select_round_view": [_vp, _c.c_int, _c.c_int64, _c.c_int32, _c.POINTER(_c.c_void_p), _i64p, _i64p, _i64p, _i32p, _i64p],
    "sdpcut_round_view": [_vp, _dp, _c.c_int, _c.c_int64, _c.c_int32, _c.POINTER(_c.c_void_p), _i64p, _i64p, _i64p, _i32p, _i64p],
    "sdpcut_round_csr": [_vp, _dp, _c.c_int, _c.c_int64, _c.POINTER(RoundCsr)],
    "sdpcut_round_csr_begin": [_vp, _dp, _c.c_int, _c.c_int64],
    "sdpcut_round_csr_end": [_vp, _c.POINTER(RoundCsr)],
    "sdpcut_score_points": [_vp, _c.c_int32, _dp, _c.c_int64, _c.c_uint32, _dp, _dp],
    "sdpcut_round_csr_points": [_vp, _c.c_int32, _dp, _c.c_int64, _c.c_int, _c.c_int64, _c.POINTER(RoundCsr)],
    "sdpcut_score_points_boxed": [_vp, _c.c_int32, _dp, _c.c_int64, _dp, _dp, _c.c_int64, _c.c_uint32, _dp, _dp],
    "sdpcut_round_csr_points_boxed": [_vp, _c.c_int32, _dp, _c.c_int64, _dp, _dp, _c.c_int64, _c.c_int, _c.c_int64, _c.POINTER(RoundCsr)],
    "sdpcut_round_csr_diverse": [_vp, _dp, _c.c_int, _c.c_int64, _c.c_int64, _c.c_double, _c.POINTER(RoundCsr), _c.POINTER(DiverseInfo)],
    "sdpcut_filter_parallel": [_vp, _c.c_int64, _i64p, _c.c_int64, _c.c_double, _c.POINTER(_c.c_uint8), _c.POINTER(DiverseInfo)],
    "sdpcut_efficacy_points": [_vp, _c.c_int32, _dp, _c.c_int64, _dp, _dp, _dp],
    "sdpcut_round_csr_points_diverse": [_vp, _c.c_int32, _dp, _c.c_int64, _dp, _dp, _c.c_int64, _c.c_int, _c.c_int64, _c.c_int64, _c.c_double,
                                        _c.POINTER(RoundCsr), _c.POINTER(DiverseInfo)],
    "sdpcut_round_csr_multi": [_vp, _dp, _c.c_int, _c.c_int64, _c.c_int32, _c.c_int64, _c.POINTER(RoundMulti)],
    "sdpcut_cut_rows_all": [_vp, _c.c_int64, _i64p, _c.c_int32, _i64p, _dp, _dp, _dp, _i64p, _i32p],
    "sdpcut_pool_create": [_vp, _c.c_int64],
    "sdpcut_pool_destroy": [_vp],
    "sdpcut_pool_add_csr": [_vp, _c.c_int64, _i32p, _i32p, _dp, _dp, _i32p, _i64p],
    "sdpcut_pool_step": [_vp, _dp, _c.POINTER(PoolParams), _c.POINTER(PoolStep)],
    "sdpcut_pool_get": [_vp, _c.c_int64, _i64p, _i64p, _i64p, _i32p, _i32p, _i32p, _i32p, _dp, _dp, _i32p, _dp],
    "sdpcut_pool_separate_points": [_vp, _c.c_int32, _dp, _c.c_int64, _c.c_uint32, _c.c_double, _c.c_int64, _c.POINTER(PoolSep)],
    "sdpcut_pool_drop": [_vp, _c.c_int64, _i64p, _i64p],
    "sdpcut_node_eval_points": [_vp, _c.c_int32, _dp, _c.c_int64, _dp, _dp, _c.c_int32, _c.c_int32, _c.c_double, _c.POINTER(NodeEval)],
    "sdpcut_dense_round": [_vp, _dp, _c.POINTER(DenseRound)],
    "sdpcut_dense_eig": [_vp, _dp, _dp],
    "sdpcut_shard_head_device": [_vp, _c.c_int, _c.c_int64, _vp],
    "sdpcut_shard_finish_enqueue": [_vp, _c.c_int32, _c.c_int64, _c.c_int32, _vp, _c.c_int64, _c.c_int64, _c.c_int32],
    "sdpcut_shard_finish_wait": [_vp, _c.c_int32, _c.POINTER(_c.c_void_p), _i64p],
    "sdpcut_shard_finish_round": [_vp, _c.c_int32, _c.c_int64, _vp, _c.c_int64, _c.c_int32, _i64p, _i64p, _dp, _dp, _dp, _dp, _i32p],
    "sdpcut_shard_finish_round_view": [_vp, _c.c_int32, _c.c_int64, _vp, _c.c_int64, _c.c_int32, _c.POINTER(_c.c_void_p)],
    "sdpcut_shard_finish_round_own": [_vp, _c.c_int32, _c.c_int64, _vp, _c.c_int64, _c.c_int32, _c.POINTER(_c.c_void_p), _i64p],
    "sdpcut_eig_batch": [_vp, _c.c_int, _c.c_int64, _dp, _dp, _dp, _dp],
    "sdpcut_nn_batch": [_vp, _c.c_int, _c.c_int64, _dp, _dp],
    "sdpcut_sdp_batch": [_vp, _c.c_int, _c.c_int64, _dp, _dp, _dp, _dp, _dp, _i32p],
    "sdpcut_train_set_data": [_vp, _c.c_int, _c.c_int64, _dp, _dp],
    "sdpcut_train_loss_grad": [_vp, _c.c_int, _c.c_int, _i32p, _dp, _c.c_int64, _c.c_int64, _c.c_int64, _dp, _dp],
    "sdpcut_last_timing": [_vp, _dp, _c.c_int],
    "sdpcut_mfma_probe": [_vp, _dp, _dp, _dp],
    "sdpcut_tri_preprocess": [_vp, _c.POINTER(_c.c_uint8), _i64p],
    "sdpcut_tri_get_triples": [_vp, _i32p, _c.POINTER(_c.c_uint8)],
    "sdpcut_tri_separate": [_vp, _c.c_int64, _i64p, _dp, _i64p, _i64p],
    "sdpcut_tri_round_csr": [_vp, _dp, _c.c_int64, _c.POINTER(TriCsr)],
    "sdpcut_tri_round_csr_points": [_vp, _c.c_int32, _dp, _c.c_int64, _dp, _dp, _c.c_int64, _c.POINTER(TriCsr)],
    "sdpcut_enumerate_cover": [_c.c_int32, _c.POINTER(_c.c_uint8), _c.c_int32, _c.c_int64, _i32p, _i32p, _i64p],
    "sdpcut_enumerate_cover_ch": [_c.c_int32, _c.POINTER(_c.c_uint8), _c.POINTER(_c.c_uint8), _c.c_int32, _c.c_int64, _i32p, _i32p, _i64p],
    "sdpcut_chordal_extension": [_c.c_int32, _c.POINTER(_c.c_uint8), _i32p, _c.POINTER(_c.c_uint8), _i32p, _i64p],
}
_RESTYPES = {"sdpcut_last_error": _c.c_char_p}
# the reference's own FFI (cut_select_qp.py:297-303): ALL that libsdpcut_nns.so exports (include/sdpcut_nns.h)
COMPAT_SYMBOLS = ["neural_net_2D", "neural_net_3D", "neural_net_4D", "neural_net_5D", "NNs_initialize", "NNs_terminate"]

_lib = None


def _torch_installed():
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return sys.modules["torch"] is not None
    try:
        return importlib.util.find_spec("torch") is not None
    except (ImportError, ValueError):
        return False


def load_library(path=None):
    """dlopen the HIP library; raises RuntimeError if it has not been built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or LIB_PATH
    # PyTorch-ROCm bundles its own HIP/HSA runtime (same SONAME libamdhip64.so.7).  A process must hold exactly
    # one of them: where torch is installed it is imported first, so that this library binds to the runtime torch
    # (device memory, streams, torch.distributed/RCCL for the sharded rounds) brings in.  Where it is not -- the
    # reference itself needs numpy and ctypes only (cut_select_qp.py:1-14, requirements.txt) -- the library binds to the
    # system ROCm named in its RUNPATH: the single-GPU product has no torch dependency; `distributed.py` is the one
    # module that imports it.
    if _torch_installed():
        import torch  # noqa: F401
    if not os.path.exists(path):
        raise RuntimeError(
            "%s not found: build it with `python -m sdpcutsel_via_nn_amd.build` "
            "(there is no CPU fallback for the cut-scoring path)" % path)
    lib = ctypes.CDLL(path)
    for name, args in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = _RESTYPES.get(name, _c.c_int)
    _lib = lib
    return lib


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a, typ):
    return a.ctypes.data_as(typ) if a is not None else None


def _view(ptr, dtype, count, shape=None):
    """``count`` items of ``dtype`` at address ``ptr`` (memory the library owns) as a numpy array, no copy; an empty array for
    a null pointer or no items"""
    if not ptr or count == 0:
        return np.zeros(shape if shape else 0, dtype=dtype)
    a = np.frombuffer((_c.c_char * (count * np.dtype(dtype).itemsize)).from_address(ptr), dtype=dtype, count=count)
    return a.reshape(shape) if shape else a


def _counters(cnt):
    """the four counters of a ranking (sdpcut_rank, the ``counters`` of sdpcut_round_csr_t) by name"""
    return dict(nb_violated=int(cnt[0]), strong=int(cnt[1]), violated=int(cnt[2]), nb_positive=int(cnt[3]))


def _empty_round():
    """the arrays of a round without a head (fresh ones: callers may keep and change what they get)"""
    z = np.zeros
    return dict(idx=z(0, np.int64), score=z(0), lam=z(0), ks=z(0, np.int32), set_inds=z((0, 5), np.int32),
                row_entry=z(0, np.int32), indptr=z(1, np.int32), indices=z(0, np.int32), values=z(0), rhs=z(0))


# the arrays of a round inside the batch block of round_csr_points: (key, record field, dtype, item size)
_BATCH_ARRAYS = (("idx", "idx", np.int64, 8), ("score", "score", np.float64, 8), ("lam", "lam_min", np.float64, 8), ("ks", "ks", np.int32, 4),
                 ("set_inds", "set_inds", np.int32, 4), ("row_entry", "row_entry", np.int32, 4), ("indptr", "indptr", np.int32, 4),
                 ("indices", "indices", np.int32, 4), ("values", "values", np.float64, 8), ("rhs", "rhs", np.float64, 8))


class SdpCutError(RuntimeError):
    pass


def check_diverse_args(max_parallel, quota, pool_size=None, strat=None):
    """The refusals of the diverse selection that need no device (the library repeats them): -> (max_parallel, quota, pool_size)."""
    mp = float(max_parallel)
    if not 0.0 <= mp <= 1.0:      # (NaN fails both comparisons)
        raise ValueError("max_parallel must lie in [0, 1]")
    quota = int(quota)
    if quota < 1:
        raise ValueError("the quota (sel_size) must be >= 1")
    if strat is not None and strat not in (STRAT_FEAS, STRAT_OPT, STRAT_COMB, STRAT_EFF):
        raise ValueError("diverse selection serves strategies 1 (feasibility), 2 (optimality), 4 (combined) and 6 (efficacy)")
    if pool_size is None:
        pool_size = min(4 * quota, DIVERSE_MAX_POOL)
        if quota > DIVERSE_MAX_POOL:
            raise ValueError("sel_size must not exceed %d" % DIVERSE_MAX_POOL)
    pool_size = int(pool_size)
    if pool_size < quota:
        raise ValueError("pool_size must be >= sel_size")
    if pool_size > DIVERSE_MAX_POOL:
        raise ValueError("pool_size must not exceed %d" % DIVERSE_MAX_POOL)
    return mp, quota, pool_size


def check_multi_args(cuts_per_set, row_quota, sel_size=None, strat=None):
    """The refusals of the multi-cut calls that need no device (the library repeats them): -> (cuts_per_set, row_quota).
    row_quota None = sel_size (the LP gets as many rows as from a plain round at most), "sets" = cuts_per_set * sel_size (every
    selected set keeps all the cuts it offers)."""
    m = int(cuts_per_set)
    if m != cuts_per_set or not 1 <= m <= MULTI_MAX_PER_SET:
        raise ValueError("cuts_per_set must be an integer in 1 .. %d" % MULTI_MAX_PER_SET)
    if strat is not None and strat not in (STRAT_FEAS, STRAT_OPT, STRAT_EXACT, STRAT_COMB, STRAT_EFF):
        raise ValueError("multi-cut rounds serve strategies 1 (feasibility), 2 (optimality), 3 (exact, with OPT_EXACT_SDP), 4 (combined) and 6 (efficacy)")
    if row_quota is None or (isinstance(row_quota, str) and row_quota == "sets"):
        if sel_size is None:
            raise ValueError("row_quota needs a number where there is no sel_size")
        q = int(sel_size) * (m if row_quota == "sets" else 1)
    elif isinstance(row_quota, str):
        raise ValueError('row_quota must be a number, None or "sets"')
    else:
        q = int(row_quota)
    if q < 1:
        raise ValueError("row_quota must be >= 1")
    return m, q


def check_pool_params(tight_tol, viol_tol, max_age, drop_age, max_return):
    """The refusals of a cut-pool step that need no device (the library repeats them)
    -> (tight_tol, viol_tol, max_age, drop_age, max_return)."""
    tt, vt = float(tight_tol), float(viol_tol)
    if not (0.0 <= tt < float("inf") and 0.0 <= vt < float("inf")):      # (NaN fails the comparisons)
        raise ValueError("tight_tol and viol_tol must be finite and >= 0")
    ma, da, mr = int(max_age), int(drop_age), int(max_return)
    if ma != max_age or da != drop_age or ma < 1 or da < 1:
        raise ValueError("max_age and drop_age must be integers >= 1")
    if mr != max_return or mr < 0:
        raise ValueError("max_return must be an integer >= 0")
    return tt, vt, ma, da, mr


_POOL_SEP_STATES = {"all": POOL_SEP_LP | POOL_SEP_PARKED, "lp": POOL_SEP_LP, "parked": POOL_SEP_PARKED}


def pool_sep_slice_bytes(cap):
    """bytes of one point's slice of the block pool_separate_points returns, for ``cap`` rows (csrc/pool_points_layout.h)"""
    cap = int(cap)
    o = 64 + cap * 8 * 3 + cap * 8 * ROW_LD + (cap + 1) * 4 + cap * 4 + cap * 4 * ROW_LD
    return (o + 63) & ~63


def check_pool_sep_args(n_points, max_return, viol_tol, states, n_rows):
    """The refusals of pool_separate_points that need no device (the library repeats them); n_rows: the rows of the pool
    -> (max_return, viol_tol, state_mask)."""
    vt = check_pool_params(0.0, viol_tol, 1, 1, 0)[1]
    mr = int(max_return)
    if mr != max_return or not 0 <= mr <= POOL_SEP_MAX_RETURN:
        raise ValueError("max_return must be an integer in 0 .. %d" % POOL_SEP_MAX_RETURN)
    if not isinstance(states, str) or states not in _POOL_SEP_STATES:
        raise ValueError('states must be "all", "parked" or "lp"')
    if not 1 <= int(n_points) <= BATCH_MAX_POINTS:
        raise ValueError("1 .. %d points per call" % BATCH_MAX_POINTS)
    cap = min(mr, int(n_rows))
    total = int(n_points) * pool_sep_slice_bytes(cap)
    if total > POOL_SEP_MAX_BLOCK_BYTES:
        raise ValueError("the result block of %d points x %d bytes (%d rows each) = %d bytes exceeds the limit of %d bytes (256 MiB)"
                         % (n_points, pool_sep_slice_bytes(cap), cap, total, POOL_SEP_MAX_BLOCK_BYTES))
    return mr, vt, _POOL_SEP_STATES[states]


def check_pool_serials(serials):
    """the serials of a pool_drop -> contiguous int64 [m] (ValueError for anything but a flat list of integers)"""
    a = np.asarray(serials)
    if a.size == 0:
        return np.zeros(0, dtype=np.int64)
    if a.ndim != 1 or a.dtype.kind not in "iu":
        raise ValueError("serials must be a flat list of integers")
    return np.ascontiguousarray(a, dtype=np.int64)


def check_pool_rows(indptr, indices, values, rhs, sense, ncols, room):
    """A block of rows for a cut pool, checked as sdpcut_pool_add_csr checks it (ValueError, nothing changed)
    -> (indptr int32, indices int32, values f64, rhs f64, sense int32), contiguous."""
    indptr = np.ascontiguousarray(indptr, dtype=np.int32)
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    values, rhs = _f64(values), _f64(rhs)
    m = rhs.shape[0]
    if indptr.ndim != 1 or indptr.shape[0] != m + 1 or rhs.ndim != 1 or indices.ndim != 1 or values.shape != indices.shape:
        raise ValueError("rows must be CSR arrays: indptr [m + 1], indices / values [nnz], rhs [m]")
    sense = np.ones(m, dtype=np.int32) if sense is None else np.ascontiguousarray(sense, dtype=np.int32)
    if sense.shape != (m,) or not np.all(np.abs(sense) == 1):
        raise ValueError("sense must be +1 (G) or -1 (L) per row")
    if m == 0:
        return indptr, indices, values, rhs, sense
    if m > room:
        raise ValueError("the block would exceed the pool's capacity")
    if indptr[0] < 0 or indptr[-1] > indices.shape[0]:
        raise ValueError("indptr does not fit indices")
    lens = np.diff(indptr)
    if lens.min() < 1:
        raise ValueError("a pool row must have at least one entry")
    if lens.max() > ROW_LD:
        raise ValueError("a pool row must have at most %d entries" % ROW_LD)
    used = slice(int(indptr[0]), int(indptr[-1]))
    if indices[used].min() < 0 or indices[used].max() >= ncols:
        raise ValueError("a column index lies outside the LP's columns")
    if not (np.all(np.isfinite(values[used])) and np.all(np.isfinite(rhs))):
        raise ValueError("a coefficient or right-hand side is not finite")
    return indptr, indices, values, rhs, sense


def _adj_u8(adjacency, n=None):
    adj = np.ascontiguousarray(np.asarray(adjacency) != 0, dtype=np.uint8)
    if adj.ndim != 2 or adj.shape[0] != adj.shape[1] or (n is not None and adj.shape[0] != n):
        raise ValueError("adjacency must be square" if n is None else "adjacency must be [n, n]")
    return adj


_u8p = _c.POINTER(_c.c_uint8)


def chordal_extension(adjacency, order=None):
    """Chordal extension of a sparsity pattern by the elimination game (sdpcut_chordal_extension; replaces chompack's symbolic
    factorisation, cut_select_qp.py:386-396).  order: a permutation of 0..n-1 to eliminate in (the reference's own AMD permutation
    reproduces the reference's pattern); None = greedy minimum degree on the elimination graph, ties to the lowest index.
    -> (ext bool [n, n]: original edges plus fill, zero diagonal; order int32 [n]: the order used; number of fill edges)."""
    lib = load_library()
    adj = _adj_u8(adjacency)
    n = adj.shape[0]
    if order is not None:
        order = np.ascontiguousarray(order, dtype=np.int32)
        if order.shape != (n,):
            raise ValueError("order must be a permutation of 0..n-1")
    ext = np.zeros((n, n), dtype=np.uint8)
    used = np.zeros(n, dtype=np.int32)
    fill = _c.c_int64(0)
    rc = lib.sdpcut_chordal_extension(n, adj.ctypes.data_as(_u8p), _ptr(order, _i32p), ext.ctypes.data_as(_u8p), _ptr(used, _i32p),
                                      ctypes.byref(fill))
    if rc != 0:
        raise ValueError("sdpcut_chordal_extension: 2 <= n <= 1024 and order must be a permutation of 0..n-1")
    return ext.astype(bool), used, int(fill.value)


def _cover_patterns(adj, dim, ch_ext, order):
    """(extended pattern | None, dim checked) for a ch_ext of 1, 2 or -1"""
    if ch_ext not in (1, 2, -1):
        raise ValueError("ch_ext must be 0 (P^E), 1 (P^bar(E)), 2 (bar(P*_3)) or -1 (P^E+_3)")
    if ch_ext in (2, -1) and int(dim) != 3:
        raise ValueError("ch_ext = 2 and ch_ext = -1 are covers of dimension 3 only")
    if ch_ext == -1:
        return None
    return np.ascontiguousarray(chordal_extension(adj, order)[0], dtype=np.uint8)


def enumerate_cover(adjacency, dim, max_subs=None, ch_ext=0, order=None):
    """Index sets of the semidefinite vertex cover P^E_dim in the reference's order
    (cut_select_qp.py:399-524).  adjacency: [n, n] array, non-zero = edge.
    -> (set_inds int32 [N, 5] padded with -1, ks int32 [N], N).  If max_subs is given and
    N >= max_subs only the count is returned (arrays None), like the reference's RAM guard.

    ch_ext (cut_select_qp.py:385-455): 1 = P^bar(E)_dim, the same cover on the chordal extension of the pattern
    (:func:`chordal_extension` with ``order``); 2 = bar(P*_3), the triangles of the extension with at least 2 original edges and
    the original edges in none (sdpcut_enumerate_cover_ch); -1 = P^E+_3, all triples.  2 and -1 need dim = 3: the reference
    silently degrades ch_ext = 2 to ch_ext = 1 at dim 4 and 5, here it is refused."""
    lib = load_library()
    adj = _adj_u8(adjacency)
    n = adj.shape[0]
    if ch_ext == 0:
        def call(max_out, sets, ks, cnt):
            return lib.sdpcut_enumerate_cover(n, adj.ctypes.data_as(_u8p), int(dim), max_out, sets, ks, cnt)
    else:
        ext = _cover_patterns(adj, dim, ch_ext, order)
        if ch_ext == 1:      # any dim: the enumeration of ch_ext = 0 on the extended pattern
            def call(max_out, sets, ks, cnt):
                return lib.sdpcut_enumerate_cover(n, ext.ctypes.data_as(_u8p), int(dim), max_out, sets, ks, cnt)
        else:
            def call(max_out, sets, ks, cnt):
                return lib.sdpcut_enumerate_cover_ch(n, ext.ctypes.data_as(_u8p) if ext is not None else None, adj.ctypes.data_as(_u8p),
                                                     int(ch_ext), max_out, sets, ks, cnt)
    cnt = _c.c_int64(0)
    rc = call(0, None, None, ctypes.byref(cnt))
    if rc != 0:
        raise ValueError("sdpcut_enumerate_cover: bad arguments (dim must be 3..5)")
    N = cnt.value
    if max_subs is not None and N >= max_subs:
        return None, None, N
    sets = np.empty((max(N, 1), 5), dtype=np.int32)
    ks = np.empty(max(N, 1), dtype=np.int32)
    rc = call(N, _ptr(sets, _i32p), _ptr(ks, _i32p), ctypes.byref(cnt))
    assert rc == 0 and cnt.value == N
    return sets[:N], ks[:N], N


class Scorer(object):
    """One handle of the C-ABI = one GPU.  Thin: argument marshalling and error mapping only
    (status codes -> ValueError / RuntimeError, SURVEY.md section 8 b)."""

    def __init__(self, device_id=0):
        self._lib = load_library()
        self._h = _vp()
        rc = self._lib.sdpcut_create(int(device_id), ctypes.byref(self._h))
        if rc != 0:
            msg = self._lib.sdpcut_last_error(None).decode()
            self._h = None
            raise SdpCutError("sdpcut_create failed (%d): %s" % (rc, msg))
        self.N = 0
        self.nb_vars = 0
        self.base = 0
        self._train_count = {}   # samples of the resident training set per candidate size (train_set_data)
        self.round_count = 0     # rounds that wrote the handle's pinned host block (views of it are good until the next one)

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc):
        if rc == 0:
            return
        msg = self._lib.sdpcut_last_error(self._h).decode()
        if rc == -1:
            raise ValueError(msg)
        raise SdpCutError("sdpcut error %d: %s" % (rc, msg))

    def _open(self):
        if getattr(self, "_h", None) is None:
            raise SdpCutError("the Scorer is closed")

    def _point_len(self):
        """length of an LP point [X packed | x]: n(n+1)/2 + n"""
        n = self.nb_vars
        return n * (n + 1) // 2 + n

    def _point(self, vars_values):
        vv = _f64(vars_values)
        if vv.shape != (self._point_len(),):
            raise ValueError("vars_values must be [X packed | x] of length n(n+1)/2 + n")
        return vv

    def close(self):
        if getattr(self, "_h", None):
            self._lib.sdpcut_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, option, value):
        self._check(self._lib.sdpcut_set_option(self._h, option, int(value)))

    def set_stream(self, stream_ptr):
        """stream_ptr: a hipStream_t as int (0 = the null stream, PyTorch's default stream);
        None restores the handle's own stream."""
        arg = _vp(-1 & 0xFFFFFFFFFFFFFFFF) if stream_ptr is None else (_vp(stream_ptr) if stream_ptr else None)
        self._check(self._lib.sdpcut_set_stream(self._h, arg))

    def get_stat(self, which):
        v = _c.c_int64(0)
        self._check(self._lib.sdpcut_get_stat(self._h, int(which), ctypes.byref(v)))
        return int(v.value)

    def filter_margin(self, k):
        """the proven bound on |y32 - y64| of the fp32 filter of the k-variable network that holds for every candidate
        (sdpcut_get_filter_margin; the filter decides by a margin per candidate that is never above it); NaN if that network does
        not filter"""
        v = _c.c_double(0.0)
        self._check(self._lib.sdpcut_get_filter_margin(self._h, int(k), ctypes.byref(v)))
        return float(v.value)

    def filter_audit(self):
        """the filter's fp32 network output, unmapped, of every candidate of a 3-variable list at the current point
        (sdpcut_filter_audit) -> float64 [N]"""
        y = np.empty(self.N, dtype=np.float64)
        self._check(self._lib.sdpcut_filter_audit(self._h, _ptr(y, _dp)))
        return y

    def filter_audit_margins(self):
        """filter_audit, and the margin the filter decides by for every candidate, each a proven bound on that candidate's
        |y32 - y64| and never above filter_margin(3) (sdpcut_filter_audit_margins) -> (y32, m), float64 [N] each"""
        y = np.empty(self.N, dtype=np.float64)
        m = np.empty(self.N, dtype=np.float64)
        self._check(self._lib.sdpcut_filter_audit_margins(self._h, _ptr(y, _dp), _ptr(m, _dp)))
        return y, m

    def wake(self):
        """an empty kernel on the handle's stream (sdpcut_wake): poke an idle device while the LP solution is still being extracted"""
        self._check(self._lib.sdpcut_wake(self._h))

    def synchronize(self):
        self._check(self._lib.sdpcut_synchronize(self._h))

    # ------------------------------------------------------------------ setup
    def set_network(self, k, widths, params):
        widths = np.ascontiguousarray(widths, dtype=np.int32)
        params = _f64(params)
        self._check(self._lib.sdpcut_set_network(self._h, int(k), widths.shape[0], _ptr(widths, _i32p),
                                                 _ptr(params, _dp), params.shape[0]))

    def set_instance(self, nb_vars, Q_arr):
        Q_arr = _f64(Q_arr)
        if Q_arr.shape != (nb_vars * (nb_vars + 1) // 2,):
            raise ValueError("Q_arr must hold the packed upper triangle, n(n+1)/2 entries")
        self.objective_key = None      # (an objective vector belongs to the instance it was set for: the library drops it)
        self._check(self._lib.sdpcut_set_instance(self._h, int(nb_vars), _ptr(Q_arr, _dp)))
        self.nb_vars = int(nb_vars)

    def set_candidates(self, set_inds, ks, global_base=0):
        set_inds = np.ascontiguousarray(set_inds, dtype=np.int32)
        ks = np.ascontiguousarray(ks, dtype=np.int32)
        if set_inds.ndim != 2 or ks.shape != (set_inds.shape[0],):
            raise ValueError("set_inds must be [N, ld] and ks [N]")
        self._check(self._lib.sdpcut_set_candidates(self._h, set_inds.shape[0], _ptr(set_inds, _i32p),
                                                    set_inds.shape[1], _ptr(ks, _i32p), int(global_base)))
        self.N = int(set_inds.shape[0])
        self.base = int(global_base)
        kmax = int(ks.max()) if ks.size else 2
        self.row_len = kmax * (kmax + 3) // 2

    def set_builtin_networks(self, max_k=5):
        """the reference's four trained MLPs, from the copy compiled into the library"""
        self._check(self._lib.sdpcut_set_builtin_networks(self._h, int(max_k)))

    def set_candidates_philox(self, k, count, seed=7, first_id=0):
        """C4 workload: `count` random k-variable index sets generated on the device, candidate ids
        first_id .. first_id + count - 1 (= the global indices reported)"""
        self._check(self._lib.sdpcut_set_candidates_philox(self._h, int(k), int(count), int(seed), int(first_id)))
        self.N, self.base = int(count), int(first_id)
        self.row_len = int(k) * (int(k) + 3) // 2

    def set_candidates_cover(self, adjacency, dim, max_subs=0, ch_ext=0, order=None):
        """semidefinite vertex cover enumerated on the device into this handle's list
        -> number of candidates (with max_subs > 0 and count >= max_subs the list is NOT replaced).
        ch_ext, order: the covers on a chordal extension, as in :func:`enumerate_cover` (sdpcut_set_candidates_cover_ch)"""
        adj = np.ascontiguousarray(np.asarray(adjacency) != 0, dtype=np.uint8)
        if adj.shape != (self.nb_vars, self.nb_vars):
            raise ValueError("adjacency must be [n, n]")
        cnt = _c.c_int64(0)
        if ch_ext == 0:
            self._check(self._lib.sdpcut_set_candidates_cover(self._h, adj.ctypes.data_as(_c.POINTER(_c.c_uint8)), int(dim),
                                                              int(max_subs or 0), ctypes.byref(cnt)))
        else:
            ext = _cover_patterns(adj, dim, ch_ext, order)
            self._check(self._lib.sdpcut_set_candidates_cover_ch(self._h, ext.ctypes.data_as(_u8p) if ext is not None else None,
                                                                 adj.ctypes.data_as(_u8p), int(ch_ext), int(dim), int(max_subs or 0),
                                                                 ctypes.byref(cnt)))
        if not (max_subs and cnt.value >= max_subs):
            self.N, self.base = int(cnt.value), 0
            self.row_len = int(dim) * (int(dim) + 3) // 2      # upper bound: the largest size present is <= dim
        return int(cnt.value)

    def set_candidates_cover_split(self, other, adjacency_obj, adjacency_all, dim):
        """The two covers of a QCQP instance (cut_select_qcqp.py:314-334) on the device: this handle gets the sub-problems
        of the cover of `adjacency_all` that also belong to the cover of `adjacency_obj`, `other` the rest
        -> (count of this handle, count of `other`)"""
        ao = np.ascontiguousarray(np.asarray(adjacency_obj) != 0, dtype=np.uint8)
        aa = np.ascontiguousarray(np.asarray(adjacency_all) != 0, dtype=np.uint8)
        if ao.shape != (self.nb_vars, self.nb_vars) or aa.shape != ao.shape:
            raise ValueError("adjacency must be [n, n]")
        n_in, n_out = _c.c_int64(0), _c.c_int64(0)
        u8 = _c.POINTER(_c.c_uint8)
        self._check(self._lib.sdpcut_set_candidates_cover_split(self._h, other._h, ao.ctypes.data_as(u8), aa.ctypes.data_as(u8), int(dim),
                                                                ctypes.byref(n_in), ctypes.byref(n_out)))
        for sc, n in ((self, n_in.value), (other, n_out.value)):
            sc.N, sc.base = int(n), 0
            sc.row_len = int(dim) * (int(dim) + 3) // 2
        return int(n_in.value), int(n_out.value)

    def get_candidates(self, local_idx):
        """-> (set_inds int32 [count, 5] padded with -1, ks int32 [count]) of candidates by local index"""
        self.drop_pending()      # (lists that live on the device are read through their scorer whenever somebody indexes them)
        idx = np.ascontiguousarray(local_idx, dtype=np.int64)
        out = np.empty((max(idx.shape[0], 1), 5), dtype=np.int32)
        ks = np.empty(max(idx.shape[0], 1), dtype=np.int32)
        self._check(self._lib.sdpcut_get_candidates(self._h, idx.shape[0], _ptr(idx, _i64p), _ptr(out, _i32p), _ptr(ks, _i32p)))
        return out[:idx.shape[0]], ks[:idx.shape[0]]

    def set_point(self, vars_values):
        vv = self._point(vars_values)
        self._check(self._lib.sdpcut_set_point(self._h, _ptr(vv, _dp)))

    def point_buffer(self):
        """The handle's pinned staging block for the LP point as a numpy array of n(n+1)/2 + n doubles: fill it in place
        and pass IT to set_point / select_round / round_csr -- the library then skips its host copy of the point."""
        p = _dp()
        self._check(self._lib.sdpcut_point_buffer(self._h, ctypes.byref(p)))
        count = self._point_len()
        addr = ctypes.cast(p, _vp).value
        return np.frombuffer((_c.c_double * count).from_address(addr), dtype=np.float64, count=count)

    def set_point_device(self, dev_ptr):
        self._check(self._lib.sdpcut_set_point_device(self._h, _vp(dev_ptr)))

    # ------------------------------------------------------------------ node box
    def set_box(self, lb, ub):
        """The variable bounds lb <= x <= ub of a branch-and-bound node (sdpcut_set_box): from here on the optimality measures
        (NN, SDP) are those of the node's small SDP -- computed on the instance tables re-expressed in the box's variables,
        :mod:`nodebox` -- while lambda_min, the violated test and the cut rows stay those of the original point.  Both None clears
        the box.  0 <= lb < ub <= 1 with ub - lb >= 2^-10, else ValueError."""
        if lb is None and ub is None:
            return self.clear_box()
        if lb is None or ub is None:
            raise ValueError("lb and ub must both be given (or both be None: clear_box)")
        from .nodebox import check_box
        lb, ub = check_box(self.nb_vars, lb, ub)
        self._check(self._lib.sdpcut_set_box(self._h, _ptr(lb, _dp), _ptr(ub, _dp)))

    def clear_box(self):
        self._check(self._lib.sdpcut_set_box(self._h, None, None))

    @property
    def box(self):
        """(lb, ub) of the node box, or None when none is set"""
        lb, ub, flag = np.empty(self.nb_vars), np.empty(self.nb_vars), _c.c_int(0)
        self._check(self._lib.sdpcut_get_box(self._h, _ptr(lb, _dp), _ptr(ub, _dp), ctypes.byref(flag)))
        return (lb, ub) if flag.value else None

    def box_tables(self, point=True):
        """-> (Q', vars') as the scoring kernels read them while a box is set (sdpcut_get_box_tables); vars' is None with
        point=False (a handle without a current LP point has none)"""
        n = self.nb_vars
        Qb = np.empty(n * (n + 1) // 2)
        vb = np.empty(self._point_len()) if point else None
        self._check(self._lib.sdpcut_get_box_tables(self._h, _ptr(Qb, _dp), _ptr(vb, _dp)))
        return Qb, vb

    # ------------------------------------------------------------------ hot path
    def score(self, flags):
        self._check(self._lib.sdpcut_score(self._h, int(flags)))

    def get_scores(self, eig=True, obj=True):
        e = np.empty(self.N) if eig else None
        o = np.empty(self.N) if obj else None
        self._check(self._lib.sdpcut_get_scores(self._h, _ptr(e, _dp), _ptr(o, _dp)))
        return e, o

    def get_sdp_scores(self):
        """-> (exact optimality measure [N], duality gap [N] in the normalised units of p*) of the last score(SDP)"""
        o, g = np.empty(self.N), np.empty(self.N)
        self._check(self._lib.sdpcut_get_sdp_scores(self._h, _ptr(o, _dp), _ptr(g, _dp)))
        return o, g

    def set_objective(self, obj):
        """The LP objective vector in the column layout of an LP point, n(n+1)/2 + n entries (sdpcut_set_objective): what the
        objective parallelism of the efficacy measure is taken against.  None clears it.  A wrong length, a non-finite entry or an
        all-zero vector is a ValueError."""
        self.objective_key = None      # (what the handle holds is unknown while the call can still fail)
        if obj is None:
            self._check(self._lib.sdpcut_set_objective(self._h, 0, None))
            return
        obj = _f64(obj)
        if obj.ndim != 1:
            raise ValueError("obj must be a vector in the layout of vars_values, n(n+1)/2 + n entries")
        self._check(self._lib.sdpcut_set_objective(self._h, obj.shape[0], _ptr(obj, _dp)))
        self.objective_key = obj.tobytes()

    objective_key = None      # the bytes of the objective vector the handle holds (set_objective), None: none, or not known

    def set_efficacy_weight(self, w):
        """w >= 0 of escore = eff + w objpar (sdpcut_set_efficacy_weight); 0, the default, ranks by pure efficacy"""
        self._check(self._lib.sdpcut_set_efficacy_weight(self._h, float(w)))

    def get_efficacy(self):
        """-> (eff, objpar, escore), float64 [N] each, of the last score(EFF) at the current point (:mod:`efficacy` is the twin)"""
        e, p, s = np.empty(self.N), np.empty(self.N), np.empty(self.N)
        self._check(self._lib.sdpcut_get_efficacy(self._h, _ptr(e, _dp), _ptr(p, _dp), _ptr(s, _dp)))
        return e, p, s

    def rank(self, strat, sel_size=0, max_out=None):
        """-> (idx int64[w], score float64[w], n_total, new_strat, counters dict)"""
        cap = self.N if max_out is None else max(0, min(int(max_out), self.N))
        idx = np.empty(max(cap, 1), dtype=np.int64)
        sc = np.empty(max(cap, 1), dtype=np.float64)
        n_total = _c.c_int64(0)
        new_strat = _c.c_int32(0)
        cnt = np.zeros(4, dtype=np.int64)
        self._check(self._lib.sdpcut_rank(self._h, int(strat), int(sel_size), cap, _ptr(idx, _i64p), _ptr(sc, _dp),
                                          ctypes.byref(n_total), ctypes.byref(new_strat), _ptr(cnt, _i64p)))
        w = min(cap, n_total.value)
        return idx[:w], sc[:w], int(n_total.value), int(new_strat.value), _counters(cnt)

    def rank_fetch(self, offset, count):
        idx = np.empty(max(count, 1), dtype=np.int64)
        sc = np.empty(max(count, 1), dtype=np.float64)
        self._check(self._lib.sdpcut_rank_fetch(self._h, int(offset), int(count), _ptr(idx, _i64p), _ptr(sc, _dp)))
        return idx[:count], sc[:count]

    def rank_device(self, strat, sel_size, max_out, d_idx_ptr, d_score_ptr):
        n_written, n_total, new_strat = _c.c_int64(0), _c.c_int64(0), _c.c_int32(0)
        cnt = np.zeros(4, dtype=np.int64)
        self._check(self._lib.sdpcut_rank_device(self._h, int(strat), int(sel_size), int(max_out), _vp(d_idx_ptr),
                                                 _vp(d_score_ptr), ctypes.byref(n_written), ctypes.byref(n_total),
                                                 ctypes.byref(new_strat), _ptr(cnt, _i64p)))
        return int(n_written.value), int(n_total.value), int(new_strat.value), _counters(cnt)

    def merge_topk_device(self, count, d_scores_ptr, d_ids_ptr, max_out, d_score_out_ptr, d_id_out_ptr,
                          d_secondary_ptr=None):
        self._check(self._lib.sdpcut_merge_topk_device(
            self._h, int(count), _vp(d_scores_ptr), _vp(d_secondary_ptr) if d_secondary_ptr else None,
            _vp(d_ids_ptr), int(max_out), _vp(d_score_out_ptr), _vp(d_id_out_ptr)))

    def gather_scores_device(self, count, d_ids_ptr, d_eig_out_ptr=None, d_obj_out_ptr=None):
        self._check(self._lib.sdpcut_gather_scores_device(
            self._h, int(count), _vp(d_ids_ptr), _vp(d_eig_out_ptr) if d_eig_out_ptr else None,
            _vp(d_obj_out_ptr) if d_obj_out_ptr else None))

    def cut_rows(self, local_idx):
        idx = np.ascontiguousarray(local_idx, dtype=np.int64)
        c = idx.shape[0]
        lam = np.empty(c)
        coef = np.empty((c, ROW_LD))
        rhs = np.empty(c)
        cols = np.empty((c, ROW_LD), dtype=np.int64)
        ks = np.empty(c, dtype=np.int32)
        self._check(self._lib.sdpcut_cut_rows(self._h, c, _ptr(idx, _i64p), _ptr(lam, _dp), _ptr(coef, _dp),
                                              _ptr(rhs, _dp), _ptr(cols, _i64p), _ptr(ks, _i32p)))
        return lam, coef, rhs, cols, ks

    def select_round(self, strat, sel_size, copy=True, point=None):
        """score (if needed) + rank + cut rows of the head in one call
        -> dict(idx, score, lam, coef, rhs, ks, n_total, new_strat, counters).

        point: the LP point [X packed | x] of this round -- set_point and the round in ONE library call
        (sdpcut_round_view).

        The device writes the results into a pinned host block owned by the handle
        (sdpcut_select_round_view).  copy=False returns numpy views of that block: no host copy
        at all, valid until the next call on this Scorer; copy=True (default) detaches them."""
        ld = self.row_len
        self.round_count += 1
        st = getattr(self, "_sr_out", None)
        if st is None:      # the out-parameters of the call, made once per Scorer (a round is a few microseconds of host time)
            block, cap, n_out, n_total, new_strat = _c.c_void_p(), _c.c_int64(0), _c.c_int64(0), _c.c_int64(0), _c.c_int32(0)
            cnt = np.zeros(4, dtype=np.int64)
            st = self._sr_out = (block, cap, n_out, n_total, new_strat, cnt,
                                 (ctypes.byref(block), ctypes.byref(cap), ctypes.byref(n_out), ctypes.byref(n_total), ctypes.byref(new_strat),
                                  _ptr(cnt, _i64p)))
        block, cap, n_out, n_total, new_strat, cnt, refs = st
        if point is not None:
            vv = self._csr_point(point)
            self._check(self._lib.sdpcut_round_view(self._h, _ptr(vv, _dp), int(strat), int(sel_size), ld, *refs))
        else:
            self._check(self._lib.sdpcut_select_round_view(self._h, int(strat), int(sel_size), ld, *refs))
        w, c = int(n_out.value), int(cap.value)
        if block.value and c:
            key = (block.value, c, ld)
            if getattr(self, "_round_view_key", None) != key:       # the block is reused round after round
                nbytes = 64 + c * 8 * (4 + ld) + c * 4
                buf = (_c.c_char * nbytes).from_address(block.value)
                o = 64
                v_idx = np.frombuffer(buf, dtype=np.int64, count=c, offset=o); o += 8 * c
                v_sc = np.frombuffer(buf, dtype=np.float64, count=c, offset=o); o += 8 * c
                v_lam = np.frombuffer(buf, dtype=np.float64, count=c, offset=o); o += 8 * c
                v_rhs = np.frombuffer(buf, dtype=np.float64, count=c, offset=o); o += 8 * c
                v_coef = np.frombuffer(buf, dtype=np.float64, count=c * ld, offset=o).reshape(c, ld); o += 8 * c * ld
                v_ks = np.frombuffer(buf, dtype=np.int32, count=c, offset=o)
                self._round_views, self._round_view_key = (v_idx, v_sc, v_lam, v_rhs, v_coef, v_ks), key
            if getattr(self, "_round_slices_w", None) != (key, w):      # (the head usually has the same length round after round)
                self._round_slices, self._round_slices_w = tuple(a[:w] for a in self._round_views), (key, w)
            idx, sc, lam, rhs, coef, ks = self._round_slices
            if copy:
                idx, sc, lam, rhs, coef, ks = (a.copy() for a in (idx, sc, lam, rhs, coef, ks))
        else:
            idx, sc, lam, rhs = np.empty(0, np.int64), np.empty(0), np.empty(0), np.empty(0)
            coef, ks = np.empty((0, ld)), np.empty(0, np.int32)
        return dict(idx=idx, score=sc, lam=lam, coef=coef, rhs=rhs, ks=ks,
                    n_total=int(n_total.value), new_strat=int(new_strat.value), counters=_counters(cnt))

    def round_csr(self, strat, sel_size, point=None, copy=False):
        """One round with the cuts assembled on the device (sdpcut_round_csr): LP point -> score -> rank -> eigen-cuts
        of the head as ONE CSR block -> dict(idx, score, lam, ks, set_inds [., 5], n_total, new_strat, counters,
        row_entry, indptr, indices, values, rhs).  The arrays are numpy views of the handle's pinned host block (written
        by the device, valid until the next call on this Scorer); copy=True detaches them.  point=None keeps the
        current LP point."""
        vv = self._csr_point(point)
        self.round_count += 1
        out = self._csr_out()
        self._check(self._lib.sdpcut_round_csr(self._h, _ptr(vv, _dp), int(strat), int(sel_size), ctypes.byref(out)))
        return self._csr_unpack(out, copy)

    def round_csr_begin(self, strat, sel_size, point=None):
        """First half of round_csr (sdpcut_round_csr_begin): enqueue the whole round, do not wait.  Several Scorers may begin
        before any ends; their device work overlaps."""
        vv = self._csr_point(point)
        self.round_count += 1
        self._check(self._lib.sdpcut_round_csr_begin(self._h, _ptr(vv, _dp), int(strat), int(sel_size)))
        self.pending = object()          # identifies THIS begun round until it is ended (or dropped)
        return self.pending

    def round_csr_end(self, copy=False):
        """Second half of round_csr (sdpcut_round_csr_end): wait for the round begun on this Scorer; the same dict."""
        out = self._csr_out()
        self.pending = None
        self._check(self._lib.sdpcut_round_csr_end(self._h, ctypes.byref(out)))
        return self._csr_unpack(out, copy)

    pending = None

    def drop_pending(self):
        """end a begun round nobody will collect (its results are discarded); True if there was one"""
        if self.pending is None:
            return False
        self.round_csr_end()
        return True

    def _csr_point(self, point):
        return None if point is None else self._point(point)

    def _csr_out(self):
        out = getattr(self, "_csr_struct", None)
        if out is None:
            out = self._csr_struct = RoundCsr()
        return out

    def _csr_unpack(self, out, copy, row_cap=None):
        """sdpcut_round_csr_t -> the round dict: the one place that maps the record.  row_cap: the capacity of the row arrays where
        it is not the head's (a multi-cut round holds up to cuts_per_set rows per entry)."""
        c, w, r = int(out.cap), int(out.n_out), int(out.n_rows)
        if c and out.idx:
            ld, rc = int(out.row_ld), c if row_cap is None else int(row_cap)
            # (plain and multi-cut rounds lay the same block out differently: the first, a middle and the last array pin the layout)
            key = (out.idx, out.ks, out.indices, c, ld, rc)
            if getattr(self, "_csr_view_key", None) != key:       # the block is reused round after round
                self._csr_views = dict(
                    idx=_view(out.idx, np.int64, c), score=_view(out.score, np.float64, c), lam=_view(out.lam_min, np.float64, c),
                    ks=_view(out.ks, np.int32, c), set_inds=_view(out.set_inds, np.int32, 5 * c, (c, 5)),
                    row_entry=_view(out.row_entry, np.int32, rc), indptr=_view(out.indptr, np.int32, rc + 1),
                    indices=_view(out.indices, np.int32, rc * ld), values=_view(out.values, np.float64, rc * ld),
                    rhs=_view(out.rhs, np.float64, rc))
                self._csr_view_key = key
            v = self._csr_views
            nnz = int(out.nnz)
            res = dict(idx=v["idx"][:w], score=v["score"][:w], lam=v["lam"][:w], ks=v["ks"][:w], set_inds=v["set_inds"][:w],
                       row_entry=v["row_entry"][:r], indptr=v["indptr"][:r + 1], indices=v["indices"][:nnz],
                       values=v["values"][:nnz], rhs=v["rhs"][:r])
            if copy:
                res = {k: a.copy() for k, a in res.items()}
        else:
            res = _empty_round()
        res.update(n_total=int(out.n_total), new_strat=int(out.new_strat), counters=_counters(out.counters))
        return res

    # ------------------------------------------------------------------ diverse selection
    @staticmethod
    def _diverse_info(info):
        return dict(pool=int(info.pool), examined=int(info.examined), skipped_nonviolated=int(info.skipped_nonviolated),
                    rejected_parallel=int(info.rejected_parallel))

    def round_csr_diverse(self, point, strat, sel_size, max_parallel, pool_size=None, copy=False):
        """One round with a parallelism filter on the ranked head (sdpcut_round_csr_diverse): the first ``pool_size`` entries of the
        strategy's ranking (default ``min(4 * sel_size, 16384)``) are walked in rank order and an entry is accepted only while fewer
        than ``sel_size`` are and its cut has ``|cos| <= max_parallel`` with every cut accepted before it.  -> the dict of
        :meth:`round_csr` for the accepted entries (every one with its row) plus ``info = dict(pool, examined, skipped_nonviolated,
        rejected_parallel)``.  point=None keeps the current LP point; strategies 1, 2 and 4."""
        mp, sel_size, pool_size = check_diverse_args(max_parallel, sel_size, pool_size, strat)
        vv = self._csr_point(point)
        self._open()
        self.round_count += 1
        out, info = self._csr_out(), DiverseInfo()
        self._check(self._lib.sdpcut_round_csr_diverse(self._h, _ptr(vv, _dp), int(strat), sel_size, pool_size, mp, ctypes.byref(out),
                                                       ctypes.byref(info)))
        res = self._csr_unpack(out, copy)
        res["info"] = self._diverse_info(info)
        return res

    def filter_parallel(self, ids, quota, max_parallel):
        """The same walk over candidates in the CALLER's order (sdpcut_filter_parallel; local ids, at the current LP point)
        -> (keep bool [count], info dict as in :meth:`round_csr_diverse`)."""
        mp, quota, _ = check_diverse_args(max_parallel, quota, DIVERSE_MAX_POOL)
        idx = np.ascontiguousarray(ids, dtype=np.int64)
        if idx.ndim != 1 or idx.shape[0] > DIVERSE_MAX_POOL:
            raise ValueError("ids must be a list of at most %d local candidate ids" % DIVERSE_MAX_POOL)
        self._open()
        keep =np.zeros(max(idx.shape[0], 1), dtype=np.uint8)
        info = DiverseInfo()
        self._check(self._lib.sdpcut_filter_parallel(self._h, idx.shape[0], _ptr(idx, _i64p), quota, mp, keep.ctypes.data_as(_u8p),
                                                     ctypes.byref(info)))
        return keep[:idx.shape[0]].astype(bool), self._diverse_info(info)

    # ------------------------------------------------------------------ all violated eigen-cuts of a set
    def round_csr_multi(self, point, strat, sel_size, cuts_per_set, row_quota=None, copy=False):
        """One round that emits up to ``cuts_per_set`` eigen-cuts per selected set (sdpcut_round_csr_multi; the rule is DESIGN.md
        section 5 "All violated eigen-cuts"): the head of :meth:`round_csr`, every entry offering its eigenpairs with eigenvalue
        < -1e-15 in ascending order, rows numbered in (entry, eigenvalue) order and those numbered >= ``row_quota`` dropped
        (None: sel_size, "sets": cuts_per_set * sel_size).  -> the dict of :meth:`round_csr` plus ``row_lam`` [rows], ``row_rank``
        [rows], ``n_neg`` [entries], ``n_used`` (entries that have a row) and ``quota_hit``.  cuts_per_set = 1 is :meth:`round_csr`
        bit for bit.  point=None keeps the current LP point; views as there unless copy=True."""
        m, quota = check_multi_args(cuts_per_set, row_quota, sel_size, strat)
        vv = self._csr_point(point)
        self._open()
        self.round_count += 1
        out = RoundMulti()
        self._check(self._lib.sdpcut_round_csr_multi(self._h, _ptr(vv, _dp), int(strat), int(sel_size), m, quota, ctypes.byref(out)))
        res = self._csr_unpack(out.csr, copy, row_cap=out.row_cap)
        w, r = res["idx"].shape[0], res["rhs"].shape[0]
        extra = dict(n_neg=_view(out.n_neg, np.int32, w), row_lam=_view(out.row_lam, np.float64, r), row_rank=_view(out.row_rank, np.int32, r))
        res.update({k: a.copy() for k, a in extra.items()} if copy else extra)
        res.update(n_used=int(out.n_used), quota_hit=bool(out.quota_hit), row_cap=int(out.row_cap))
        return res

    def cut_rows_all(self, local_idx, cuts_per_set):
        """Up to ``cuts_per_set`` eigen-cuts of each of the given candidates (local ids, any order, repeats allowed) at the current
        LP point (sdpcut_cut_rows_all) -> (row_ptr int64 [count + 1], row_lam [rows], coef [rows, 20], rhs [rows], cols int64
        [count, 20], ks int32 [count]): entry i owns rows row_ptr[i] .. row_ptr[i + 1] - 1, all on the columns cols[i]."""
        m, _ = check_multi_args(cuts_per_set, 1)
        idx = np.ascontiguousarray(local_idx, dtype=np.int64)
        if idx.ndim != 1:
            raise ValueError("local_idx must be a list of local candidate ids")
        self._open()
        c = idx.shape[0]
        row_ptr = np.zeros(c + 1, dtype=np.int64)
        lam = np.empty(max(c * m, 1))
        coef = np.empty((max(c * m, 1), ROW_LD))
        rhs = np.empty(max(c * m, 1))
        cols = np.empty((max(c, 1), ROW_LD), dtype=np.int64)
        ks = np.empty(max(c, 1), dtype=np.int32)
        self._check(self._lib.sdpcut_cut_rows_all(self._h, c, _ptr(idx, _i64p), m, _ptr(row_ptr, _i64p), _ptr(lam, _dp), _ptr(coef, _dp),
                                                  _ptr(rhs, _dp), _ptr(cols, _i64p), _ptr(ks, _i32p)))
        n = int(row_ptr[c])
        return row_ptr, lam[:n], coef[:n], rhs[:n], cols[:c], ks[:c]

    # ------------------------------------------------------------------ cut pool
    pool_capacity = 0

    def _pool_open(self):
        self._open()
        if not self.pool_capacity:
            raise SdpCutError("pool_create first")

    def pool_create(self, capacity):
        """A cut pool of at most ``capacity`` rows on this handle (sdpcut_pool_create; DESIGN.md section 5 "Cut pool"); needs
        set_instance.  Replaces an existing pool."""
        capacity = int(capacity)
        if not 1 <= capacity <= POOL_MAX_ROWS:
            raise ValueError("capacity must lie in 1 .. %d" % POOL_MAX_ROWS)
        self._open()
        self._check(self._lib.sdpcut_pool_create(self._h, capacity))
        self.pool_capacity, self._pool_rows = capacity, 0

    def pool_destroy(self):
        if getattr(self, "_h", None) is not None:
            self._check(self._lib.sdpcut_pool_destroy(self._h))
        self.pool_capacity, self._pool_rows = 0, 0

    def pool_add(self, indptr, indices, values, rhs, sense=None):
        """Rows (host CSR arrays; sense +1 "G" / -1 "L" per row, None = all "G") enter the pool in the LP with age 0
        (sdpcut_pool_add_csr) -> the serial of the first one; the others follow it.  A refused block (ValueError) leaves the pool
        unchanged."""
        self._pool_open()
        indptr, indices, values, rhs, sense = check_pool_rows(indptr, indices, values, rhs, sense, self._point_len(),
                                                              self.pool_capacity - self._pool_rows)
        first = _c.c_int64(0)
        self._check(self._lib.sdpcut_pool_add_csr(self._h, rhs.shape[0], _ptr(indptr, _i32p), _ptr(indices, _i32p), _ptr(values, _dp),
                                                  _ptr(rhs, _dp), _ptr(sense, _i32p), ctypes.byref(first)))
        self._pool_rows += rhs.shape[0]
        return int(first.value)

    def pool_step(self, point=None, tight_tol=1e-9, viol_tol=1e-6, max_age=3, drop_age=10, max_return=0, copy=True):
        """One step of the pool at an LP point (sdpcut_pool_step; point=None keeps the current one): the LP rows age and the slack
        ones are parked, the violated parked rows return most violated first, the others age and drop.
        -> dict(leave, enter, dropped: serials; enter_indptr, enter_indices, enter_values, enter_rhs, enter_sense, enter_key: the
        returning rows in rank order; n_in_lp, n_parked (after the step), n_violated (before the cap max_return), n_dropped).
        copy=False returns views of the pool's pinned block, valid until the next pool call."""
        self._pool_open()
        tt, vt, ma, da, mr = check_pool_params(tight_tol, viol_tol, max_age, drop_age, max_return)
        vv = self._csr_point(point)
        par, out = PoolParams(tt, vt, ma, da, mr), PoolStep()
        self._check(self._lib.sdpcut_pool_step(self._h, _ptr(vv, _dp), ctypes.byref(par), ctypes.byref(out)))

        w, nnz = int(out.n_enter), int(out.enter_nnz)
        self._pool_rows -= int(out.n_dropped)
        res = dict(leave=_view(out.leave, np.int64, int(out.n_leave)), enter=_view(out.enter, np.int64, w),
                   dropped=_view(out.dropped, np.int64, int(out.n_dropped)),
                   enter_indptr=_view(out.enter_indptr, np.int32, w + 1) if w else np.zeros(1, np.int32),
                   enter_indices=_view(out.enter_indices, np.int32, nnz), enter_values=_view(out.enter_values, np.float64, nnz),
                   enter_rhs=_view(out.enter_rhs, np.float64, w), enter_sense=_view(out.enter_sense, np.int32, w),
                   enter_key=_view(out.enter_key, np.float64, w))
        if copy:
            res = {k: a.copy() for k, a in res.items()}
        res.update(n_in_lp=int(out.n_in_lp), n_parked=int(out.n_parked), n_violated=int(out.n_violated), n_dropped=int(out.n_dropped))
        return res

    def pool_state(self):
        """The whole pool in row order (sdpcut_pool_get), for tests and tools -> dict(n, next_serial, serial, state, age, nnz,
        sense, rhs, norm, cols [n, 20], vals [n, 20])."""
        self._pool_open()
        n, nxt = _c.c_int64(0), _c.c_int64(0)
        self._check(self._lib.sdpcut_pool_get(self._h, 0, ctypes.byref(n), ctypes.byref(nxt), *([None] * 11)))
        m = int(n.value)
        a = dict(serial=np.zeros(m, np.int64), state=np.zeros(m, np.int32), age=np.zeros(m, np.int32), nnz=np.zeros(m, np.int32),
                 sense=np.zeros(m, np.int32), rhs=np.zeros(m), norm=np.zeros(m), cols=np.zeros((m, ROW_LD), np.int32),
                 vals=np.zeros((m, ROW_LD)))
        if m:
            self._check(self._lib.sdpcut_pool_get(self._h, m, ctypes.byref(n), ctypes.byref(nxt), _ptr(a["serial"], _i64p),
                                                  _ptr(a["state"], _i32p), _ptr(a["age"], _i32p), _ptr(a["nnz"], _i32p),
                                                  _ptr(a["sense"], _i32p), _ptr(a["rhs"], _dp), _ptr(a["norm"], _dp),
                                                  _ptr(a["cols"], _i32p), _ptr(a["vals"], _dp)))
        a.update(n=m, next_serial=int(nxt.value))
        return a

    def pool_separate_points(self, points, max_return, viol_tol=1e-6, states="all", copy=False):
        """The pool separated at P LP points in one call with one host wait, READ-ONLY (sdpcut_pool_separate_points): points
        [P, n(n+1)/2 + n] (a view whose rows lie further apart than their length is passed as it is).  ``states``: the rows examined
        -- "all" (a global pool), "parked" or "lp".  -> list of P dicts: the first min(max_return, n_violated) rows violated by
        more than ``viol_tol * ||row||`` at the point, by (key descending, serial ascending): serial, key, indptr, indices, values,
        rhs, sense; n_violated (before the cap; max_return = 0 returns the counts alone) and select_passes (0: the violated rows
        fitted the workgroup's list).  The pool, the Scorer's point, scores and box stay as they were.  Views of the pool's pinned
        block, valid until the next pool call (copy=True detaches them)."""
        self._pool_open()
        pts = np.asarray(points)
        n = self._point_len()
        if not (pts.dtype == np.float64 and pts.ndim == 2 and pts.shape[1] == n and pts.shape[0] >= 1 and pts.strides[1] == 8
                and (pts.shape[0] == 1 or (pts.strides[0] % 8 == 0 and pts.strides[0] >= 8 * n))):
            pts = _f64(points)
        if pts.ndim != 2 or pts.shape[1] != n:
            raise ValueError("points must be [P, n(n+1)/2 + n]: one LP point [X packed | x] per row")
        P = pts.shape[0]
        mr, vt, mask = check_pool_sep_args(P, max_return, viol_tol, states, self._pool_rows)
        recs = (PoolSep * P)()
        self._check(self._lib.sdpcut_pool_separate_points(self._h, P, _ptr(pts, _dp), pts.strides[0] // 8 if P > 1 else n, mask, vt, mr, recs))
        res = []
        for o in recs:
            w, nnz = int(o.n_rows), int(o.nnz)
            d = dict(serial=_view(o.serial, np.int64, w), key=_view(o.key, np.float64, w),
                     indptr=_view(o.indptr, np.int32, w + 1) if o.indptr else np.zeros(1, np.int32),
                     indices=_view(o.indices, np.int32, nnz), values=_view(o.values, np.float64, nnz),
                     rhs=_view(o.rhs, np.float64, w), sense=_view(o.sense, np.int32, w))
            if copy:
                d = {k: a.copy() for k, a in d.items()}
            d.update(n_violated=int(o.n_violated), select_passes=int(o.select_passes))
            res.append(d)
        return res

    def pool_drop(self, serials):
        """The rows with these serials leave the pool (sdpcut_pool_drop): any order, duplicates count once, serials not in the pool
        are ignored; the rows behind a removed row move up, serials are never reused -> the number removed."""
        self._pool_open()
        ser = check_pool_serials(serials)
        gone = _c.c_int64(0)
        self._check(self._lib.sdpcut_pool_drop(self._h, ser.shape[0], _ptr(ser, _i64p), ctypes.byref(gone)))
        self._pool_rows -= int(gone.value)
        return int(gone.value)

    def node_eval_points(self, points, boxes=None, max_sweeps=50, branch_rule=1, rho=0.2, copy=True):
        """What a tree node needs after its LP solves, at P LP points in one launch with one host wait, READ-ONLY
        (sdpcut_node_eval_points; :mod:`nodeeval` states the rule and is the numpy twin, equal bit for bit): points
        [P, n(n+1)/2 + n], boxes [P, 2, n] = (lb, ub) of every point's node or None (the unit box).  Needs :meth:`set_objective`.
        -> dict of x_local [P, n], f_point, f_local, branch_score, branch_val (float64 [P]), sweeps, moves, branch_var (int32 [P];
        -1: no variable is wide enough to branch on).  The Scorer's point, scores, box, pending round and pool stay as they were.
        copy=False: x_local is a strided view of the handle's pinned block, valid until the next call of this method."""
        pts = _f64(points)
        if pts.ndim != 2 or pts.shape[1] != self._point_len():
            raise ValueError("points must be [P, n(n+1)/2 + n]: one LP point [X packed | x] per row")
        n, P = int(self.nb_vars), pts.shape[0]
        if not 1 <= P <= BATCH_MAX_POINTS:
            raise ValueError("1 .. %d points per call" % BATCH_MAX_POINTS)
        lb = ub = None
        if boxes is not None:
            bx = _f64(boxes)
            if bx.shape != (P, 2, n):
                raise ValueError("boxes must be [P, 2, n]: (lb, ub) per point")
            lb, ub = _f64(bx[:, 0, :]), _f64(bx[:, 1, :])
        if int(max_sweeps) != max_sweeps or not 0 <= max_sweeps <= 2 ** 31 - 1:
            raise ValueError("max_sweeps must be an integer >= 0")
        if int(branch_rule) != branch_rule or abs(int(branch_rule)) > 2 ** 30:
            raise ValueError("branch_rule must be 0 or 1")
        recs = (NodeEval * P)()
        self._check(self._lib.sdpcut_node_eval_points(self._h, P, _ptr(pts, _dp), pts.shape[1], _ptr(lb, _dp), _ptr(ub, _dp), int(max_sweeps),
                                                      int(branch_rule), float(rho), recs))
        slice_d = ((64 + 8 * n + 63) // 64) * 8      # doubles of a point's slice: a 64-byte header, x_local [n], padded to 64 bytes
        xl = _view(recs[0].x_local, np.float64, (P - 1) * slice_d + n)
        xl = np.lib.stride_tricks.as_strided(xl, shape=(P, n), strides=(8 * slice_d, 8), writeable=False)
        return dict(x_local=xl.copy() if copy else xl,
                    f_point=np.array([o.f_point for o in recs]), f_local=np.array([o.f_local for o in recs]),
                    sweeps=np.array([o.sweeps for o in recs], np.int32), moves=np.array([o.moves for o in recs], np.int32),
                    branch_var=np.array([o.branch_var for o in recs], np.int32),
                    branch_score=np.array([o.branch_score for o in recs]), branch_val=np.array([o.branch_val for o in recs]))

    # ------------------------------------------------------------------ many LP points per call
    def _points_arg(self, points):
        pts = _f64(points)
        if pts.ndim != 2 or pts.shape[1] != self._point_len():
            raise ValueError("points must be [P, n(n+1)/2 + n]: one LP point [X packed | x] per row")
        if not 1 <= pts.shape[0] <= BATCH_MAX_POINTS:
            raise ValueError("1 .. %d points per call" % BATCH_MAX_POINTS)
        return pts

    def _boxes_arg(self, pts, boxes):
        """boxes [P, 2, n] of a boxed batch, checked (nodebox.check_boxes) -> contiguous float64, and the pointers (lb, ub, box_ld)
        the boxed entry points take"""
        from .nodebox import check_boxes
        bx = check_boxes(self.nb_vars, boxes, n_points=pts.shape[0])
        n = int(self.nb_vars)
        ub = _c.cast(_c.c_void_p(bx.ctypes.data + 8 * n), _dp)
        return bx, bx.ctypes.data_as(_dp), ub, 2 * n

    def score_points(self, points, eig=True, obj=True, boxes=None):
        """Scores of the candidate list at P LP points in one call (sdpcut_score_points): points [P, n(n+1)/2 + n] ->
        (eig [P, N] | None, obj [P, N] | None), row p = what set_point(points[p]), score, get_scores return.  Leaves the Scorer
        without a current point.
        boxes [P, 2, n]: (lb, ub) of the node of every point (sdpcut_score_points_boxed); row p is then what set_box(*boxes[p]),
        set_point, score, get_scores return.  The Scorer must have no box of its own and has none afterwards."""
        pts = self._points_arg(points)
        if not (eig or obj):
            raise ValueError("nothing asked for")
        P = pts.shape[0]
        e = np.empty((P, self.N)) if eig else None
        o = np.empty((P, self.N)) if obj else None
        flags = (EIG if eig else 0) | (NN if obj else 0)
        if boxes is None:
            self._check(self._lib.sdpcut_score_points(self._h, P, _ptr(pts, _dp), pts.shape[1], flags, _ptr(e, _dp), _ptr(o, _dp)))
        else:
            bx, lb, ub, box_ld = self._boxes_arg(pts, boxes)
            self._check(self._lib.sdpcut_score_points_boxed(self._h, P, _ptr(pts, _dp), pts.shape[1], lb, ub, box_ld, flags,
                                                            _ptr(e, _dp), _ptr(o, _dp)))
        return e, o

    def round_csr_points(self, points, strat, sel_size, copy=False, boxes=None):
        """P rounds with the cuts assembled, one LP point each, in one call (sdpcut_round_csr_points): points [P, n(n+1)/2 + n] ->
        list of P dicts, entry p = what round_csr(strat, sel_size, point=points[p]) returns (same keys, dtypes and values).  The
        arrays are numpy views of the handle's pinned batch block, valid until the next call on this Scorer; copy=True detaches
        them.  Strategies 1, 2 and 4.  Leaves the Scorer without a current point.
        boxes [P, 2, n]: (lb, ub) of the node of every point (sdpcut_round_csr_points_boxed); entry p is then what set_box(*boxes[p])
        followed by round_csr(strat, sel_size, point=points[p]) returns.  The Scorer must have no box of its own and has none
        afterwards."""
        pts = self._points_arg(points)
        P = pts.shape[0]
        if boxes is not None:
            bx, lb, ub, box_ld = self._boxes_arg(pts, boxes)
        self._open()
        self.round_count += 1
        recs =getattr(self, "_csr_points_recs", None)
        if recs is None or recs.shape[0] < P:
            recs = self._csr_points_recs = np.zeros(max(P, 8), dtype=_ROUND_CSR_DTYPE)
        if boxes is None:
            self._check(self._lib.sdpcut_round_csr_points(self._h, P, _ptr(pts, _dp), pts.shape[1], int(strat), int(sel_size),
                                                          recs.ctypes.data_as(_c.POINTER(RoundCsr))))
        else:
            self._check(self._lib.sdpcut_round_csr_points_boxed(self._h, P, _ptr(pts, _dp), pts.shape[1], lb, ub, box_ld, int(strat),
                                                                int(sel_size), recs.ctypes.data_as(_c.POINTER(RoundCsr))))
        return self._points_unpack(recs, P, copy)

    def _points_unpack(self, recs, P, copy):
        """the P records of a batched round -> list of P round dicts (views of the batch block, or copies)"""
        r = recs[:P]
        held = r["idx"][r["idx"] != 0]      # (a point without a head has no arrays)
        base = int(held.min()) if held.size else 0
        if base:
            # ONE byte view over the batch block (cached while the block stays where it is); every array is a slice of it
            c_max, ld = int(r["cap"].max()), int(r["row_ld"][0])
            end = int(r["indices"].max()) + 4 * c_max * ld
            key = (base, end)
            if getattr(self, "_csr_points_key", None) != key:
                self._csr_points_u8 = np.frombuffer((_c.c_char * (end - base)).from_address(base), dtype=np.uint8)
                self._csr_points_key = key
            u8 = self._csr_points_u8
        cols = {f: r[f].tolist() for f in _ROUND_CSR_DTYPE.names}
        res = []
        for p in range(P):
            c, w, nr, nnz = cols["cap"][p], cols["n_out"][p], cols["n_rows"][p], cols["nnz"][p]
            if c and cols["idx"][p]:
                counts = dict(idx=w, score=w, lam=w, ks=w, set_inds=5 * w, row_entry=nr, indptr=nr + 1, indices=nnz, values=nnz, rhs=nr)
                d = {}
                for key, field, dtype, size in _BATCH_ARRAYS:
                    o = cols[field][p] - base
                    d[key] = u8[o:o + counts[key] * size].view(dtype)
                d["set_inds"] = d["set_inds"].reshape(w, 5)
                if copy:
                    d = {k: a.copy() for k, a in d.items()}
            else:
                d = _empty_round()
            d.update(n_total=cols["n_total"][p], new_strat=cols["new_strat"][p], counters=_counters(cols["counters"][p]))
            res.append(d)
        return res

    def efficacy_points(self, points):
        """Efficacy of the candidate list at P LP points in one call (sdpcut_efficacy_points): points [P, n(n+1)/2 + n] ->
        (eff, objpar, escore), each [P, N]; row p = what set_point(points[p]), score(EIG | EFF), get_efficacy return, with the
        Scorer's objective and weight.  Leaves the Scorer without a current point."""
        pts = self._points_arg(points)
        P = pts.shape[0]
        e, o, s = np.empty((P, self.N)), np.empty((P, self.N)), np.empty((P, self.N))
        self._check(self._lib.sdpcut_efficacy_points(self._h, P, _ptr(pts, _dp), pts.shape[1], _ptr(e, _dp), _ptr(o, _dp), _ptr(s, _dp)))
        return e, o, s

    def round_csr_points_diverse(self, points, strat, sel_size, max_parallel, pool_size=None, copy=False, boxes=None):
        """P filtered rounds, one LP point each, in one call (sdpcut_round_csr_points_diverse): -> list of P dicts, entry p = what
        round_csr_diverse(points[p], strat, sel_size, max_parallel, pool_size) returns, ``info`` included; strategies 1, 2, 4 and 6.
        boxes [P, 2, n]: entry p is what set_box(*boxes[p]) followed by that call returns.  Views of the pinned batch block, valid
        until the next call on this Scorer (copy=True detaches them).  Leaves the Scorer without a current point and without a box."""
        mp, sel_size, pool_size = check_diverse_args(max_parallel, sel_size, pool_size, strat)
        pts = self._points_arg(points)
        P = pts.shape[0]
        lb = ub = None
        box_ld = 0
        if boxes is not None:
            bx, lb, ub, box_ld = self._boxes_arg(pts, boxes)
        self._open()
        self.round_count += 1
        recs = getattr(self, "_csr_points_recs", None)
        if recs is None or recs.shape[0] < P:
            recs = self._csr_points_recs = np.zeros(max(P, 8), dtype=_ROUND_CSR_DTYPE)
        infos = (DiverseInfo * P)()
        self._check(self._lib.sdpcut_round_csr_points_diverse(self._h, P, _ptr(pts, _dp), pts.shape[1], lb, ub, box_ld, int(strat), sel_size,
                                                              pool_size, mp, recs.ctypes.data_as(_c.POINTER(RoundCsr)), infos))
        res = self._points_unpack(recs, P, copy)
        for p in range(P):
            res[p]["info"] = self._diverse_info(infos[p])
        return res

    # ------------------------------------------------------------------ dense eigen-cuts (strategy 0)
    def dense_round(self, point=None, copy=False):
        """Dense eigen-cuts of the whole lifted matrix at the LP point (sdpcut_dense_round; strategy 0, cut_select_qp.py:757-786)
        -> dict(eigvals [n+1] ascending, n_rows, sweeps, cols [row_len] shared by all rows, values [n_rows, row_len], rhs [n_rows]).
        Needs set_instance and a point only.  The arrays are numpy views of the handle's pinned host block (valid until the next
        call on this Scorer); copy=True detaches them.  point=None keeps the current LP point."""
        vv = self._csr_point(point)
        self.round_count += 1
        out = DenseRound()
        self._check(self._lib.sdpcut_dense_round(self._h, _ptr(vv, _dp), ctypes.byref(out)))
        D, r, rl = int(out.dim), int(out.n_rows), int(out.row_len)
        res = dict(eigvals=_view(out.eigvals, np.float64, D), cols=_view(out.cols, np.int32, rl),
                   values=_view(out.values, np.float64, r * rl, (r, rl)), rhs=_view(out.rhs, np.float64, r))
        if copy:
            res = {k: a.copy() for k, a in res.items()}
        res.update(n_rows=r, sweeps=int(out.sweeps))
        return res

    def dense_eig(self, vectors=False):
        """Eigen-decomposition of the whole lifted matrix at the current point (sdpcut_dense_eig): eigenvalues ascending
        [n+1], and with vectors=True also V [n+1, n+1] with V[:, j] the unit vector of eigenvalue j (numpy.linalg.eigh's layout)."""
        D = self.nb_vars + 1
        w = np.empty(D)
        v = np.empty((D, D)) if vectors else None
        self._check(self._lib.sdpcut_dense_eig(self._h, _ptr(w, _dp), _ptr(v, _dp)))
        return (w, v) if vectors else w

    # ------------------------------------------------------------------ sharded round (multi-GPU)
    def shard_head_device(self, strat, count, d_record_ptr):
        """enqueue this shard's packed head record (8 + 2*count int64 words); no host sync"""
        self._check(self._lib.sdpcut_shard_head_device(self._h, int(strat), int(count), _vp(d_record_ptr)))

    def _shard_views(self, block, w, m, ld):
        key = (block, w, m, ld)
        if getattr(self, "_shard_view_key", None) != key:           # the block is reused round after round
            nbytes = w * 64 + m * 8 * (4 + ld) + m * 8
            buf = (_c.c_char * nbytes).from_address(block)
            o = 0
            hdr = np.frombuffer(buf, dtype=np.int64, count=w * 8, offset=o).reshape(w, 8); o += w * 64
            idx = np.frombuffer(buf, dtype=np.int64, count=m, offset=o); o += 8 * m
            sc = np.frombuffer(buf, dtype=np.float64, count=m, offset=o); o += 8 * m
            lam = np.frombuffer(buf, dtype=np.float64, count=m, offset=o); o += 8 * m
            rhs = np.frombuffer(buf, dtype=np.float64, count=m, offset=o); o += 8 * m
            coef = np.frombuffer(buf, dtype=np.float64, count=m * ld, offset=o).reshape(m, ld); o += 8 * m * ld
            ks = np.frombuffer(buf, dtype=np.int32, count=m, offset=o); o += 4 * m
            pos = np.frombuffer(buf, dtype=np.int32, count=m, offset=o)
            self._shard_views_cache = dict(headers=hdr, idx=idx, score=sc, lam=lam, coef=coef, rhs=rhs, ks=ks, pos=pos)
            self._shard_view_key = key
        return self._shard_views_cache

    def shard_finish_enqueue(self, world, count, d_allrec_ptr, sel_size, fields=2, pitch_words=0):
        """second half of a sharded round, enqueued without host synchronisation (sdpcut_shard_finish_enqueue);
        fields = 3: the records carry obj_improve as secondary key (SDPCUT_PART_COMBALL); pitch_words: distance between
        consecutive ranks' records when several lists share the gathered buffer (0 = one list per buffer)"""
        # (the library refuses a second enqueue -- or any other stateful call -- before the wait: state changes only on success)
        self._check(self._lib.sdpcut_shard_finish_enqueue(self._h, int(world), int(count), int(fields), _vp(d_allrec_ptr),
                                                          int(pitch_words), int(sel_size), self.row_len))
        self.round_count += 1
        self._shard_pending = (int(world), int(sel_size), self.row_len)

    def shard_finish_wait(self, own=True):
        """-> dict(headers, idx, score, lam, coef, rhs, ks[, pos, n_own]): views of the handle's pinned block, which the
        device wrote (valid until the next round on this Scorer); own=True: lam / coef / rhs / ks hold only this shard's
        n_own rows, compacted in head order, pos[:n_own] their positions in the head"""
        w, m, ld = self._shard_pending
        block, n_own = _c.c_void_p(), _c.c_int64(0)
        self._check(self._lib.sdpcut_shard_finish_wait(self._h, 1 if own else 0, ctypes.byref(block), ctypes.byref(n_own)))
        out = dict(self._shard_views(block.value, w, m, ld))
        if own:
            out["n_own"] = int(n_own.value)
        else:
            out.pop("pos")
        return out

    def shard_finish_round(self, world, count, d_allrec_ptr, sel_size, copy=False):
        """merge the gathered records, cut rows of this shard's entries
        -> dict(headers [world, 8], idx, score, lam, coef, rhs, ks), each of sel_size entries:
        numpy views of the handle's pinned host block, which the device wrote directly
        (valid until the next call on this Scorer; copy=True detaches them)"""
        m, ld, w = int(sel_size), self.row_len, int(world)
        self.round_count += 1
        block = _c.c_void_p()
        self._check(self._lib.sdpcut_shard_finish_round_view(
            self._h, w, int(count), _vp(d_allrec_ptr), m, ld, ctypes.byref(block)))
        out = {k: v for k, v in self._shard_views(block.value, w, m, ld).items() if k != "pos"}
        return {k: v.copy() for k, v in out.items()} if copy else out

    def shard_finish_round_own(self, world, count, d_allrec_ptr, sel_size):
        """like shard_finish_round, but lam / coef / rhs / ks hold only the n_own rows of this shard
        (compacted in head order by the library) and pos[:n_own] their positions in the head
        -> dict(headers, idx, score, lam, coef, rhs, ks, pos, n_own); views, see above"""
        m, ld, w = int(sel_size), self.row_len, int(world)
        self.round_count += 1
        block, n_own = _c.c_void_p(), _c.c_int64(0)
        self._check(self._lib.sdpcut_shard_finish_round_own(
            self._h, w, int(count), _vp(d_allrec_ptr), m, ld, ctypes.byref(block), ctypes.byref(n_own)))
        out = dict(self._shard_views(block.value, w, m, ld))
        out["n_own"] = int(n_own.value)
        return out

    # ------------------------------------------------------------------ triangle inequalities
    def tri_preprocess(self, adjacency):
        """-> (triples int32 [T, 3], density uint8 [T]) kept on the device as well."""
        adj = np.ascontiguousarray(np.asarray(adjacency) != 0, dtype=np.uint8)
        if adj.shape != (self.nb_vars, self.nb_vars):
            raise ValueError("adjacency must be [n, n]")
        T = _c.c_int64(0)
        self._check(self._lib.sdpcut_tri_preprocess(self._h, adj.ctypes.data_as(_c.POINTER(_c.c_uint8)),
                                                    ctypes.byref(T)))
        tri = np.empty((max(T.value, 1), 3), dtype=np.int32)
        dens = np.empty(max(T.value, 1), dtype=np.uint8)
        self._check(self._lib.sdpcut_tri_get_triples(self._h, _ptr(tri, _i32p),
                                                     dens.ctypes.data_as(_c.POINTER(_c.c_uint8))))
        self.n_tri = int(T.value)
        return tri[:T.value], dens[:T.value]

    def tri_separate(self, max_out):
        """-> (entry ids 4*triple+type int64[w], violations float64[w], n_violated)"""
        cap = max(0, min(int(max_out), 4 * getattr(self, "n_tri", 0)))
        ent = np.empty(max(cap, 1), dtype=np.int64)
        vio = np.empty(max(cap, 1))
        nv, nw = _c.c_int64(0), _c.c_int64(0)
        self._check(self._lib.sdpcut_tri_separate(self._h, cap, _ptr(ent, _i64p), _ptr(vio, _dp), ctypes.byref(nv),
                                                  ctypes.byref(nw)))
        return ent[:nw.value], vio[:nw.value], int(nv.value)

    TRI_MAX_OUT = 16384      # most entries of one tri_separate / tri_round_csr call

    @staticmethod
    def _tri_unpack(rec, copy):
        """a sdpcut_tri_csr_t -> dict(entry, viol, indptr, indices, values, rhs, n_rows, n_violated): views of the pinned block, or copies"""
        r, nnz = int(rec.n_rows), int(rec.nnz)
        out = dict(entry=_view(rec.entry, np.int64, r), viol=_view(rec.viol, np.float64, r), indptr=_view(rec.indptr, np.int32, r + 1),
                   indices=_view(rec.indices, np.int32, nnz), values=_view(rec.values, np.float64, nnz), rhs=_view(rec.rhs, np.float64, r))
        if copy:
            out = dict((k, np.array(v)) for k, v in out.items())
        out.update(n_rows=r, n_violated=int(rec.n_violated))
        return out

    def tri_round_csr(self, max_out, point=None, copy=False):
        """The triangle separation with its rows assembled on the device (sdpcut_tri_round_csr): at ``point`` (None: the current one)
        the first ``max_out`` violated triangle inequalities, ranked as :meth:`tri_separate` ranks them, and their rows in the
        hand-over form of a round's cuts, sense >=.  With a node box (:meth:`set_box`) the inequalities are those of the box
        (:mod:`triangles`).  -> dict(entry int64 [r], viol [r], indptr int32 [r + 1], indices int32, values, rhs [r], n_rows,
        n_violated); the arrays are views of the handle's pinned block, valid until the next call on this Scorer (copy=True
        detaches them)."""
        if not 0 <= int(max_out) <= self.TRI_MAX_OUT:
            raise ValueError("max_out must be 0 .. %d" % self.TRI_MAX_OUT)
        rec = TriCsr()
        vv = None if point is None else self._point(point)
        self._check(self._lib.sdpcut_tri_round_csr(self._h, _ptr(vv, _dp), int(max_out), ctypes.byref(rec)))
        return self._tri_unpack(rec, copy)

    def tri_round_csr_points(self, points, max_out, boxes=None, copy=False):
        """:meth:`tri_round_csr` at P LP points in one call with one host wait (sdpcut_tri_round_csr_points): points [P, n(n+1)/2 + n]
        -> list of P dicts, entry p = what tri_round_csr(max_out, point=points[p]) returns -- with boxes [P, 2, n], inside
        set_box(*boxes[p]).  Views of the handle's pinned batch block, valid until the next call (copy=True detaches them).  The
        Scorer must have no box of its own; it is left without a current point and without a box."""
        pts = self._points_arg(points)
        P = pts.shape[0]
        if not 0 <= int(max_out) <= self.TRI_MAX_OUT:
            raise ValueError("max_out must be 0 .. %d" % self.TRI_MAX_OUT)
        lb = ub = None
        if boxes is not None:
            from .nodebox import check_boxes
            bx = check_boxes(self.nb_vars, boxes, n_points=P)
            lo, hi = np.ascontiguousarray(bx[:, 0, :]), np.ascontiguousarray(bx[:, 1, :])
            lb, ub = _ptr(lo, _dp), _ptr(hi, _dp)
        recs = (TriCsr * P)()
        self._check(self._lib.sdpcut_tri_round_csr_points(self._h, P, _ptr(pts, _dp), pts.shape[1], lb, ub, int(max_out), recs))
        return [self._tri_unpack(recs[p], copy) for p in range(P)]

    def eig_batch(self, k, x_rho, X_rho, want_vectors=False):
        x_rho, X_rho = _f64(x_rho), _f64(X_rho)
        c = x_rho.shape[0]
        if x_rho.shape != (c, k) or X_rho.shape != (c, k * (k + 1) // 2):
            raise ValueError("x_rho must be [count, k] and X_rho [count, k(k+1)/2]")
        w = np.empty((c, k + 1))
        v = np.empty((c, k + 1, k + 1)) if want_vectors else None
        self._check(self._lib.sdpcut_eig_batch(self._h, int(k), c, _ptr(x_rho, _dp), _ptr(X_rho, _dp), _ptr(w, _dp),
                                               _ptr(v, _dp)))
        return (w, v) if want_vectors else w

    def nn_batch(self, k, inputs):
        inputs = _f64(inputs)
        c = inputs.shape[0]
        if inputs.shape != (c, k * (k + 3) // 2):
            raise ValueError("inputs must be [count, k(k+3)/2]")
        out = np.empty(c)
        self._check(self._lib.sdpcut_nn_batch(self._h, int(k), c, _ptr(inputs, _dp), _ptr(out, _dp)))
        return out

    def sdp_batch(self, k, inputs, want_certificate=False):
        """Exact solve of the small SDP on explicit inputs [count, k(k+3)/2] = [x | Q_slice] (sdpcut_sdp_batch)
        -> (value = certified lower bound on p* [count], gap [count]); want_certificate=True: a dict with value, gap and the
        certificate lam [count, k], Y [count, k(k+1)/2] (upper triangle), iters int32 [count]."""
        inputs = _f64(inputs)
        c = inputs.shape[0]
        if inputs.shape != (c, k * (k + 3) // 2):
            raise ValueError("inputs must be [count, k(k+3)/2]")
        value, gap = np.empty(c), np.empty(c)
        lam = Y = iters = None
        if want_certificate:
            lam, Y, iters = np.empty((c, k)), np.empty((c, k * (k + 1) // 2)), np.empty(c, dtype=np.int32)
        self._check(self._lib.sdpcut_sdp_batch(self._h, int(k), c, _ptr(inputs, _dp), _ptr(value, _dp), _ptr(gap, _dp), _ptr(lam, _dp),
                                               _ptr(Y, _dp), _ptr(iters, _i32p)))
        if want_certificate:
            return dict(value=value, gap=gap, lam=lam, Y=Y, iters=iters)
        return value, gap

    def train_set_data(self, k, inputs, targets):
        """Make (inputs [count, k(k+3)/2] = [x | Q_slice], targets [count]) the resident training set of size k
        (sdpcut_train_set_data); an empty set drops it."""
        inputs, targets = _f64(inputs), _f64(targets)
        c = targets.shape[0]
        if inputs.shape != (c, k * (k + 3) // 2) or targets.shape != (c,):
            raise ValueError("inputs must be [count, k(k+3)/2] and targets [count]")
        self._check(self._lib.sdpcut_train_set_data(self._h, int(k), c, _ptr(inputs, _dp), _ptr(targets, _dp)))
        self._train_count[int(k)] = c

    def train_loss_grad(self, k, widths, params, first=0, count=None, want_grad=True):
        """Normalised mean squared error of the network (widths, params: the packing of set_network) over samples
        [first, first + count) of the resident set and its gradient with respect to every W and b, in the order of params
        (sdpcut_train_loss_grad) -> (loss, grad float64[n_params - (2 d_in + 4)]), grad None with want_grad=False.
        count=None: through the end of the set."""
        widths = np.ascontiguousarray(widths, dtype=np.int32)
        params = _f64(params)
        if count is None:
            count = self._train_count.get(int(k), 0) - int(first)
        loss = _c.c_double(0.0)
        d_in = int(k) * (int(k) + 3) // 2
        grad = np.empty(max(params.shape[0] - (2 * d_in + 4), 0)) if want_grad else None
        self._check(self._lib.sdpcut_train_loss_grad(self._h, int(k), widths.shape[0], _ptr(widths, _i32p), _ptr(params, _dp),
                                                     params.shape[0], int(first), int(count), ctypes.byref(loss), _ptr(grad, _dp)))
        return float(loss.value), grad

    def last_timing(self):
        ms = np.zeros(2)
        self._check(self._lib.sdpcut_last_timing(self._h, _ptr(ms, _dp), 2))
        return float(ms[0]), float(ms[1])

    def mfma_probe(self, A, B):
        A, B = _f64(A), _f64(B)
        assert A.shape == (16, 4) and B.shape == (4, 16)
        C = np.empty((16, 16))
        self._check(self._lib.sdpcut_mfma_probe(self._h, _ptr(A, _dp), _ptr(B, _dp), _ptr(C, _dp)))
        return C
