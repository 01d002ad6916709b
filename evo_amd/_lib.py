"""ctypes binding of libevo_amd.so (include/evo_amd.h).

This is the thin C-ABI layer BASELINE.json:north_star asks for: Python host code, hand-written
HIP kernels, no PyTorch.  The library must be present and a gfx950 GPU must be visible for any
compute call; there is deliberately NO CPU fallback (the CPU restatement under oracle/ is test
infrastructure and is never imported from here).
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libevo_amd.so")

MODEL_BSC, MODEL_SSSC = 0, 1

# evoamd_generate: keep bits (EVOAMD_GEN_KEEP_*) and the output ids of evoamd_download_generated (EVOAMD_GEN_*)
GEN_KEEP = {"s": 1, "z": 2, "y_mean": 4}
GEN_WHAT = {"y": 0, "s": 1, "z": 2, "y_mean": 3}

# evoamd_seed_states_ex: flags (EVOAMD_SEED_*)
SEED_INCOMPLETE = 1
# evoamd_sweep_propose_ex / evoamd_sweep_states_ex: flags (EVOAMD_SWEEP_*)
SWEEP_INCOMPLETE = 1
# evoamd_sweep_propose_nb / evoamd_sweep_states_nb: the neighbourhood bits beside it
SWEEP_SWAP, SWEEP_NO_FLIP = 2, 4
SWEEP_NEIGHBOURHOODS = {"flip": 0, "swap": SWEEP_SWAP | SWEEP_NO_FLIP, "both": SWEEP_SWAP}
# evoamd_neighbour_bound: flags (EVOAMD_NBOUND_*)
NBOUND_INCOMPLETE = 1
# evoamd_ais_loglik: flags (EVOAMD_AIS_*); evoamd_ais_posterior_ex takes AIS_INCOMPLETE alone
AIS_REVERSE, AIS_ADMIT, AIS_INCOMPLETE = 1, 2, 8

# evoamd_posterior_sample: keep bits (EVOAMD_PSAMP_KEEP_*) and the output ids of evoamd_download_posterior_samples
PSAMP_KEEP = {"slot": 1, "s": 2, "z": 4, "y": 8}
PSAMP_WHAT = {"slot": 0, "s": 1, "z": 2, "y": 3}

# evoamd_download_loglik_draws: the output ids (EVOAMD_LLE_*)
LLE_WHAT = {"s": 0, "inside": 1, "log_r": 2, "lpj": 3}

# evoamd_debug_validity: names of the bits of out[0] (EVOAMD_VB_*, in bit order) and of out[1..7]
VALIDITY_BITS = (
    "have_data", "have_params", "have_cand", "B_valid", "rows_fresh", "stats_rows_valid", "yhat_valid", "rec_resident",
    "yrec_valid", "yrec_from_pass", "rec_in_stats", "keep_x_valid", "rec_uses_keep", "need_known", "res_need0",
    "res_need1", "res_need2", "cand_from_device", "lists_clean", "clist_clean", "acc_clean", "wq_copy_valid",
    "h_theta_fresh", "theta_bak_valid", "kn_lost", "last_estep_fused", "reduce_pending", "bins_dirty", "gen_kept",
    "prefetch_current", "census_current", "rows_kn_current",
)
VALIDITY_WORDS = ("gen", "kn_gen", "theta_gen", "pending_skip", "census_skip", "kn_refill", "pred_N")

# kernel-class ids of evoamd_kernel_time_ms (evo_amd.hip: KID_*)
KERNEL_IDS = {
    "lpj_resident": 0, "lpj_candidates": 1, "lpj_overflow": 2, "row_lse": 3, "vary_kn": 4,
    "stats": 5, "stats_overflow": 6, "gemm_f64": 7, "evolve": 8, "misc": 9, "mstep_device": 10,
    "lpj_pass": 11, "stats_pass": 12, "lpj_k3_4": 13, "lpj_k5_8": 14, "lpj_k9plus": 15,
    "stats_k3_4": 16, "stats_k5_8": 17, "stats_k9plus": 18, "allreduce": 19, "estep_fused": 20,
    "patches": 21, "init_states": 22,
}
# classes outside the EM path, added after tests/test_gpu_validity.py recorded its launch census over KERNEL_IDS (which
# therefore stays as it is); Engine.timing / Engine.kernel_time_ms take names of either table
KERNEL_IDS_EXTRA = {"posterior_sample": 23, "seed_states": 24, "loglik_proposal": 25, "loglik_lpj": 26, "loglik_fold": 27,
                    "remap_latents": 28, "stats_kappa": 29, "sweep": 30, "sweep_swap": 31, "resize": 32,
                    "neighbour_bound": 33, "predictive_score": 34, "ais": 35, "ais_post": 36}


def kernel_id(name):
    return KERNEL_IDS[name] if name in KERNEL_IDS else KERNEL_IDS_EXTRA[name]

_c_dp = ctypes.POINTER(ctypes.c_double)
_c_u8p = ctypes.POINTER(ctypes.c_uint8)
_c_i32p = ctypes.POINTER(ctypes.c_int32)
_c_u64p = ctypes.POINTER(ctypes.c_uint64)
_vp = ctypes.c_void_p
_I, _I64, _U64, _DBL = ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_double



class SweepOut(ctypes.Structure):
    """evoamd_sweep_out: the outputs of the _nb sweep calls, each pointer may be NULL."""
    _fields_ = [("score", _c_dp), ("best_flip", _c_i32p), ("gain", _c_dp), ("n_capped", _c_i32p),
                ("best_swap", _c_i32p), ("swap_gain", _c_dp), ("n_capped_swap", _c_i32p)]


class NboundOut(ctypes.Structure):
    """evoamd_nbound_out: the outputs of evoamd_neighbour_bound, each pointer may be NULL."""
    _fields_ = [("F", _c_dp), ("M", _c_dp), ("n_states", _c_i32p), ("n_capped", _c_i32p), ("best_score", _c_dp),
                ("best_parent", _c_i32p), ("best_flip", _c_i32p), ("sum", _c_dp)]


class AisOut(ctypes.Structure):
    """evoamd_ais_out: the outputs of evoamd_ais_loglik, each pointer may be NULL."""
    _fields_ = [("ll", _c_dp), ("ess", _c_dp), ("log_w_mean", _c_dp), ("log_w_min", _c_dp), ("log_w_max", _c_dp),
                ("n_flips", ctypes.POINTER(ctypes.c_int64)), ("log_w", _c_dp), ("final_words", _c_u64p), ("chain_flips", _c_i32p),
                ("F_before", _c_dp), ("F_after", _c_dp), ("admit_sums", _c_dp), ("sum", _c_dp)]


class AisPostOut(ctypes.Structure):
    """evoamd_ais_post_out: the outputs of evoamd_ais_posterior, each pointer may be NULL."""
    _fields_ = [("p", _c_dp), ("p_se", _c_dp), ("count", _c_dp), ("map_lpj", _c_dp), ("map_state", _c_u64p), ("ll", _c_dp),
                ("ess", _c_dp), ("log_w_mean", _c_dp), ("log_w_min", _c_dp), ("log_w_max", _c_dp),
                ("n_flips", ctypes.POINTER(ctypes.c_int64)), ("mean", _c_dp), ("log_w", _c_dp), ("rb", _c_dp),
                ("chain_map_lpj", _c_dp), ("chain_map_state", _c_u64p), ("chain_flips", _c_i32p)]


class AisPostSelOut(ctypes.Structure):
    """evoamd_ais_post_sel_out: evoamd_ais_post_out and the outputs of EVOAMD_AIS_ADMIT, each pointer may be NULL."""
    _fields_ = [("post", AisPostOut), ("F_before", _c_dp), ("F_after", _c_dp), ("n_distinct", _c_i32p), ("n_new", _c_i32p),
                ("n_proposed", _c_i32p), ("n_admitted", _c_i32p), ("map_held_before", _c_i32p), ("map_held_after", _c_i32p),
                ("admit_sums", _c_dp)]


class PredScoreOut(ctypes.Structure):
    """evoamd_pred_score_out: the outputs of evoamd_predictive_score, each pointer may be NULL (logp and pit together)."""
    _fields_ = [("logp", _c_dp), ("pit", _c_dp), ("logp_n", _c_dp), ("count", _c_i32p)]


_I32 = ctypes.c_int32


class DenseDesc(ctypes.Structure):
    """evoamd_dense_desc: one call of the test-only evoamd_dense_probe."""
    _fields_ = [("op", _I32), ("M", _I32), ("Nc", _I32), ("K", _I64), ("lda", _I32), ("ldb", _I32), ("ldc", _I32),
                ("lda2", _I32), ("ldct", _I32), ("off_a", _I32), ("off_b", _I32), ("off_c", _I32), ("same_operand", _I32),
                ("deterministic", _I32), ("sym_row0", _I32), ("c_is_zero", _I32), ("accumulate", _I32), ("mirror", _I32),
                ("spare", _I32), ("diag", _I32), ("guard", _I32)]


class DenseRoute(ctypes.Structure):
    """evoamd_dense_route: what the dense launcher chose."""
    _fields_ = [("route", _I32), ("tile", _I32), ("splits", _I32), ("J", _I32), ("wpx", _I32), ("segmax", _I32),
                ("ws", _I32), ("n_cu", _I32)]


DENSE_OPS = ("tn", "tn_f32", "nn", "rows", "rows_f32", "colsum", "colsum_sq")  # EVOAMD_DENSE_*
DENSE_ROUTES = ("none", "gram_small", "tn64_scalar", "tn64_vec", "tn128_split", "tn128_streamk", "tn128_grouped",
                "f32_streamk", "f32_grouped", "f32_naive", "nn_small", "nn_vec", "nn_scalar", "rows", "rows_f32_store",
                "rows_f32_naive", "colsum")  # EVOAMD_ROUTE_*


# name -> (restype, argtypes); one entry per prototype in include/evo_amd.h
SIGNATURES = {
    "evoamd_abi_version": (_I, []),
    "evoamd_last_error": (ctypes.c_char_p, []),
    "evoamd_device_count": (_I, [ctypes.POINTER(_I)]),
    "evoamd_ctx_create": (_I, [_I, ctypes.POINTER(_vp)]),
    "evoamd_ctx_destroy": (None, [_vp]),
    "evoamd_synchronize": (_I, [_vp]),
    "evoamd_debug_live_buffers": (_I, [ctypes.POINTER(_I64)]),
    "evoamd_debug_validity": (_I, [_vp, ctypes.POINTER(_I64)]),
    "evoamd_set_option": (_I, [_vp, ctypes.c_char_p, _I]),
    "evoamd_configure": (_I, [_vp, _I, _I64, _I, _I, _I, _I, _I]),
    "evoamd_upload_data": (_I, [_vp, _c_dp]),
    "evoamd_upload_states": (_I, [_vp, _c_u8p]),
    "evoamd_download_states": (_I, [_vp, _c_u8p]),
    "evoamd_upload_states_packed": (_I, [_vp, _c_u8p, _I64, _I64]),
    "evoamd_download_states_packed": (_I, [_vp, _c_u8p, _I64, _I64]),
    "evoamd_init_states": (_I, [_vp, _DBL, _U64, _I, _c_u8p]),
    "evoamd_seed_states": (_I, [_vp, _I, _c_i32p, _c_dp]),
    "evoamd_seed_states_ex": (_I, [_vp, _I, ctypes.c_uint, _c_i32p, _c_dp]),
    "evoamd_seed_states_beam": (_I, [_vp, _I, _I, _c_i32p, _c_dp]),
    "evoamd_upload_lpj": (_I, [_vp, _c_dp]),
    "evoamd_download_lpj": (_I, [_vp, _c_dp]),
    "evoamd_set_params_bsc": (_I, [_vp, _c_dp, _DBL, _DBL, _c_dp]),
    "evoamd_set_params_sssc": (_I, [_vp, _c_dp, _c_dp, _c_dp, _c_dp, _DBL, _c_dp]),
    "evoamd_lpj_resident": (_I, [_vp]),
    "evoamd_lpj_candidates": (_I, [_vp, _c_u8p, _c_i32p, _I, _c_dp]),
    "evoamd_set_candidates": (_I, [_vp, _c_u8p, _c_i32p, _I, _c_dp]),
    "evoamd_lpj_shared": (_I, [_vp, _c_u8p, _I, _c_dp]),
    "evoamd_lpj_single": (_I, [_vp, _c_dp, _c_u8p, _I, _c_dp, _c_i32p]),
    "evoamd_vary_kn": (_I, [_vp, _I, _c_dp]),
    "evoamd_evolve_randflip": (_I, [_vp, _I, _I, _U64, _I]),
    "evoamd_estep": (_I, [_vp, _I, _I, _U64, _I, _I, ctypes.POINTER(_I)]),
    "evoamd_estep_counters": (_I, [_vp, ctypes.POINTER(_I64)]),
    "evoamd_evolve_states": (_I, [_vp, _I, _I, _I, _I, _I, _U64, _DBL, _DBL]),
    "evoamd_download_candidates": (_I, [_vp, _c_u8p, _c_i32p, _c_dp]),
    "evoamd_refine_states": (_I, [_vp, _I, _I, _I, _I, _I, _I, _U64, _U64, _DBL, _DBL, _I, _I, _I, _DBL, _c_dp,
                                  ctypes.POINTER(_I)]),
    "evoamd_sweep_propose": (_I, [_vp, _I, _I, _c_dp, _c_i32p, _c_dp, _c_i32p]),
    "evoamd_sweep_states": (_I, [_vp, _I, _I, _I, _I, _I, _c_dp, ctypes.POINTER(_I), _c_i32p, _c_dp, _c_i32p]),
    "evoamd_sweep_propose_ex": (_I, [_vp, _I, _I, ctypes.c_uint, _c_dp, _c_i32p, _c_dp, _c_i32p]),
    "evoamd_sweep_states_ex": (_I, [_vp, _I, _I, _I, _I, _I, ctypes.c_uint, _c_dp, ctypes.POINTER(_I), _c_i32p, _c_dp,
                                    _c_i32p]),
    "evoamd_sweep_propose_nb": (_I, [_vp, _I, _I, ctypes.c_uint, ctypes.POINTER(SweepOut)]),
    "evoamd_sweep_states_nb": (_I, [_vp, _I, _I, _I, _I, _I, ctypes.c_uint, _c_dp, ctypes.POINTER(_I),
                                    ctypes.POINTER(SweepOut)]),
    "evoamd_neighbour_bound": (_I, [_vp, _I, ctypes.c_uint, ctypes.POINTER(NboundOut)]),
    "evoamd_ais_loglik": (_I, [_vp, _I, _I, _c_dp, _U64, _U64, ctypes.c_uint, _c_u64p, _I, ctypes.POINTER(AisOut)]),
    "evoamd_ais_posterior": (_I, [_vp, _I, _I, _I, _c_dp, _U64, _U64, _I64, ctypes.POINTER(AisPostOut)]),
    "evoamd_ais_posterior_ex": (_I, [_vp, _I, _I, _I, _c_dp, _U64, _U64, _I64, ctypes.c_uint, ctypes.POINTER(AisPostOut)]),
    "evoamd_ais_posterior_sel": (_I, [_vp, _I, _I, _I, _c_dp, _U64, _U64, _I64, ctypes.c_uint, ctypes.POINTER(_I64), _I64, _I,
                                      ctypes.POINTER(AisPostSelOut)]),
    "evoamd_ais_post_admit_probe": (_I, [_vp, _c_dp, _c_u64p, _I, ctypes.POINTER(_I64), _I64, _c_i32p, _c_i32p, _c_i32p,
                                         _c_i32p, _c_u64p, ctypes.POINTER(_I)]),
    "evoamd_posterior_scores": (_I, [_vp, _c_dp, _c_dp, _c_i32p, _c_i32p, _c_dp]),
    "evoamd_remap_latents": (_I, [_vp, _c_i32p, _I, _c_i32p, ctypes.POINTER(_I64)]),
    "evoamd_adopt_remapped_states": (_I, [_vp]),
    "evoamd_resize_states": (_I, [_vp, _I, _c_i32p]),
    "evoamd_adopt_resized_states": (_I, [_vp]),
    "evoamd_latent_map_counts": (_I, [_vp, ctypes.POINTER(_I64)]),
    "evoamd_acc_size": (_I64, [_vp]),
    "evoamd_stats": (_I, [_vp, _c_dp]),
    "evoamd_mstep_device": (_I, [_vp, _I, _c_dp, _c_dp]),
    "evoamd_reconstruct": (_I, [_vp, _c_dp]),
    "evoamd_upload_masks": (_I, [_vp, _c_u8p, _c_u8p]),
    "evoamd_upload_yrec": (_I, [_vp, _c_dp]),
    "evoamd_set_reliable_fraction": (_I, [_vp, ctypes.c_double]),
    "evoamd_lpj_single_masked": (_I, [_vp, _c_dp, _c_u8p, _c_u8p, _I, _c_dp, _c_i32p]),
    "evoamd_inverse": (_I, [_vp, _c_dp, _c_dp, _I, _c_dp]),
    "evoamd_gemm_tn": (_I, [_vp, _c_dp, _c_dp, _c_dp, _I64, _I, _I, _I]),
    "evoamd_dense_probe": (_I, [_vp, ctypes.POINTER(DenseDesc), _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(DenseRoute)]),
    "evoamd_get_params_bsc": (_I, [_vp, _c_dp, _c_dp, _c_dp]),
    "evoamd_get_params_sssc": (_I, [_vp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp]),
    "evoamd_restore_theta_backup": (_I, [_vp]),
    "evoamd_free_energy": (_I, [_vp, _c_dp, _I64, _I, _c_dp]),
    "evoamd_loglik_exact": (_I, [_vp, _I, _I, _c_dp, _c_dp, _c_dp]),
    "evoamd_set_estep_counts": (_I, [_vp, _DBL, _DBL]),
    "evoamd_patches_extract": (_I, [_vp, _c_dp, _I, _I, _I, _I, _I, _I, _c_dp]),
    "evoamd_patches_merge": (_I, [_vp, _c_dp, _I, _I, _I, _I, _I, _I, _I, _c_dp]),
    "evoamd_patches_merge_weighted": (_I, [_vp, _c_dp, _c_dp, _I, _I, _I, _I, _I, _I, _c_dp]),
    "evoamd_reconstruct_resident": (_I, [_vp, _c_u8p]),
    "evoamd_patches_merge_resident": (_I, [_vp, _I, _I, _I, _I, _I, _I, _I, _c_dp]),
    "evoamd_download_reconstruction": (_I, [_vp, _c_dp]),
    "evoamd_posterior_codes": (_I, [_vp, _I, _DBL, _c_i32p, _c_dp, _c_dp, _c_i32p, _c_i32p, _c_dp, _c_u8p]),
    "evoamd_download_posterior": (_I, [_vp, _c_dp, _c_dp]),
    "evoamd_predictive_moments": (_I, [_vp, _I, ctypes.POINTER(_I64)]),
    "evoamd_download_predictive": (_I, [_vp, _c_dp, _c_dp]),
    "evoamd_predictive_score": (_I, [_vp, _c_dp, _c_u8p, _I, ctypes.POINTER(PredScoreOut), ctypes.POINTER(_I64), _c_dp]),
    "evoamd_posterior_sample": (_I, [_vp, _I, _U64, _U64, _I, _I, _I, ctypes.POINTER(_I64)]),
    "evoamd_download_posterior_samples": (_I, [_vp, _I, _vp]),
    "evoamd_loglik_estimate": (_I, [_vp, _I, _U64, _U64, _DBL, _I, _c_dp, _c_dp, _c_dp, _c_dp, _c_i32p,
                                    ctypes.POINTER(_I64), _c_dp]),
    "evoamd_download_loglik_draws": (_I, [_vp, _I, _vp]),
    "evoamd_patches_merge_samples": (_I, [_vp, _I, _I, _I, _I, _I, _I, _I, _I, _I, _c_dp, _c_dp, _c_dp]),
    "evoamd_patches_merge_predictive": (_I, [_vp, _I, _I, _I, _I, _I, _I, _I, _c_dp]),
    "evoamd_generate": (_I, [_vp, _I, _I64, _I, _I, _U64, _U64, _c_dp, _c_dp, _c_dp, _c_dp, _DBL, _c_u64p, _I]),
    "evoamd_download_generated": (_I, [_vp, _I, _vp]),
    "evoamd_comm_unique_id": (_I, [_c_u8p]),
    "evoamd_comm_init": (_I, [_vp, _c_u8p, _I, _I]),
    "evoamd_comm_allreduce_host": (_I, [_vp, _c_dp, _I64, _I]),
    "evoamd_comm_destroy": (_I, [_vp]),
    "evoamd_timing_enable": (_I, [_vp, _I]),
    "evoamd_timing_enable64": (_I, [_vp, _U64]),
    "evoamd_timing_reset": (_I, [_vp]),
    "evoamd_kernel_time_ms": (_I, [_vp, _I, _c_dp, ctypes.POINTER(_I64)]),
    "evoamd_kernel_name": (ctypes.c_char_p, [_I]),
}


class EvoAmdError(RuntimeError):
    pass


_lib = None


def load():
    """Load libevo_amd.so (once).  Raises EvoAmdError with build instructions if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EvoAmdError(
            "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C evo_amd/csrc`). evo_amd has no CPU fallback." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here == header / library mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise EvoAmdError("libevo_amd error %d: %s" % (rc, load().evoamd_last_error().decode()))


def dptr(a):
    return a.ctypes.data_as(_c_dp)


def u8ptr(a):
    return a.ctypes.data_as(_c_u8p)


def i32ptr(a):
    return a.ctypes.data_as(_c_i32p)


def as_f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def as_bool_bytes(a):
    """C-contiguous bool array viewed as uint8 (the reference's own K^n layout, 1 byte per latent)."""
    a = np.ascontiguousarray(a, dtype=np.bool_)
    return a.view(np.uint8)
