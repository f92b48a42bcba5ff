"""
Host-side mirror of the reference's operator API on top of libtftfund.so.

The reference's drop-in surface is the MATLAB calling convention
    [R_t_2, R_t_3, Reconst, T, iter] = Method(Corresp, CalM)
(experiments.m:51-59,108).  This module exposes

  * the same names with the same argument meaning for ONE triplet
    (`LinearTFTPoseEstimation(Corresp, CalM)` with Corresp 6xN, CalM 9x3), and
  * `*_batch` variants for B triplets -- the form the GPU is built for --
    on numpy arrays (host path: the library does H2D/D2H) or on torch CUDA
    tensors (device path: only pointers and the current stream are passed; torch
    is plumbing for device memory and streams, nothing else).

There is no CPU fallback: if libtftfund.so is missing or no HIP device is
present, every call raises.
"""
import ctypes
import os
import threading

import numpy as np
# torch is plumbing here (device memory, streams, torch.distributed) -- and it must be
# imported BEFORE libtftfund.so is dlopen'ed: the torch wheel bundles its own
# libamdhip64.so (soname libamdhip64.so.7); loading it first makes the dynamic loader
# bind libtftfund.so to that same HIP runtime instead of starting a second one.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libtftfund.so")

TFF_OPT_SOLVER = 1
TFF_OPT_STAGE_LDS = 2
TFF_OPT_KERNEL = 3
TFF_OPT_GH_EXACT = 4
TFF_OPT_EXACT_BELOW = 5
TFF_OPT_SPILL = 6
TFF_OPT_ROWS = 7
TFF_OPT_DEBUG_FP_HANDOVER = 8
TFF_OPT_DEBUG_ADAPTIVE = 9
TFF_OPT_PRE = 10
TFF_OPT_COUNT_ROWS = 11
TFF_OPT_BA_CLASSES = 12
TFF_OPT_SCORE = 13
SCORE_UNITS = 64             # TFF_SCORE_UNITS: the MSAC weight of a perfect inlier (count <= score <= SCORE_UNITS * count)
SCORES = {"count": 0, "msac": 1}
DEBUG_STRIDE = 128

ST_OK, ST_TOO_FEW, ST_NONFINITE, ST_NO_POSE, ST_RANK, ST_NO_PARAM = 0, 1, 2, 3, 4, 5
ST_BAD_OFFSETS = 6
ST_TOO_LARGE = 7             # ragged bundle adjustment: more selected correspondences than BA_MAX_N
BA_MAX_N = 3124              # include/tftfund.h TFF_BA_MAX_N
ROBUST_CHUNK = 262144        # hypotheses per chunk of tff_robust_pose_* (csrc/robust_kernel.h); the result does not depend on it

_c_dp = ctypes.c_void_p
_POSE_SIG = [ctypes.c_void_p, _c_dp, _c_dp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32,
             _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp]

_lib = None
_lib_lock = threading.Lock()


class TffError(RuntimeError):
    pass


def load_library(path=None):
    """dlopen libtftfund.so and declare its prototypes.  Raises if it is missing:
    the product has no other compute path."""
    global _lib
    with _lib_lock:
        if _lib is not None and path is None:
            return _lib
        p = path or _LIB_PATH
        if not os.path.exists(p):
            raise TffError("libtftfund.so not found at %s -- build it with `python -m tft_vs_fund_amd.build` "
                           "(hipcc --offload-arch=gfx950); there is no CPU fallback" % p)
        lib = ctypes.CDLL(p)
        lib.tff_version.restype = ctypes.c_int
        lib.tff_last_error.restype = ctypes.c_char_p
        lib.tff_ctx_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]
        lib.tff_ctx_destroy.argtypes = [ctypes.c_void_p]
        lib.tff_ctx_destroy.restype = None
        lib.tff_ctx_set_stream.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        lib.tff_ctx_use_own_stream.argtypes = [ctypes.c_void_p]
        lib.tff_ctx_get_stream.argtypes = [ctypes.c_void_p]
        lib.tff_ctx_get_stream.restype = ctypes.c_void_p
        lib.tff_ctx_set_option.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_long]
        lib.tff_ctx_synchronize.argtypes = [ctypes.c_void_p]
        for name in POSE_METHODS.values():
            for suffix in ("_dev", "_host"):
                fn = getattr(lib, name + suffix, None)
                if fn is not None:
                    fn.argtypes = _POSE_SIG
                    fn.restype = ctypes.c_int
        for name in POSE_METHODS.values():
            fn = getattr(lib, name + "_debug_dev", None)
            if fn is not None:
                fn.argtypes = _POSE_SIG + [_c_dp]
                fn.restype = ctypes.c_int
        V, I64, I32, F64, U64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_double, ctypes.c_uint64
        protos = {
            "tff_triangulate_batch_dev": [V, V, I64, V, I64, I32, I32, V],
            "tff_repr_error_batch_dev": [V, V, I64, V, I64, V, I64, I32, V],
            "tff_inlier_count_batch_dev": [V, V, I32, V, V, V, I64, F64, V, V],
            "tff_transform_tft_batch_dev": [V, V, V, V, V, I64, I64, I32, V],
            "tff_rt_from_tft_batch_dev": [V, V, V, I64, V, I64, I32, V, V, V],
            "tff_linear_tft_batch_dev": [V, V, I64, I32, V, V, V, V],
            "tff_linear_f_batch_dev": [V, V, I64, I32, I32, V, V, V, V],
            "tff_bundle_adjust_batch_dev": [V, V, I64, V, V, V, I64, I32, V, V, V, V, V, V, V],
            "tff_bundle_adjust_batch_host": [V, V, I64, V, V, V, I64, I32, V, V, V, V, V, V, V],
            "tff_bundle_adjust_views_batch_dev": [V, I32, V, I64, V, V, I64, I32, V, V, V, V, V, V],
            "tff_bundle_adjust_views_batch_host": [V, I32, V, I64, V, V, I64, I32, V, V, V, V, V, V],
            "tff_pi_pose_batch_debug_dev": [V, I32, V, V, I64, I64, I32, V, V, V, V, V, V, V, V],
            "tff_linear_tft_pose_sampled_dev": [V, V, I32, V, V, I64, I32, V, V, V, V],
            "tff_linear_f_pose_sampled_dev": [V, V, I32, V, V, I64, I32, V, V, V, V],
            "tff_multi_create": [ctypes.POINTER(ctypes.c_void_p), V, I32],
            "tff_pose_batch_host_multi": [V, I32, V, V, I64, I64, I32, V, V, V, V, V, V],
            "tff_pose_batch_dev_multi": [V, I32, V, V, I64, I64, I32, V, V],
            "tff_pose_batch_ragged_dev": [V, I32, V, V, I32, V, I64, I64, V, V, V, V, V, V],
            "tff_pose_batch_ragged_host": [V, I32, V, V, V, I64, I64, V, V, V, V, V, V],
            "tff_sample_indices_dev": [V, U64, I64, I64, I32, I32, V],
            "tff_inlier_mask_batch_dev": [V, V, I32, V, V, V, I64, F64, V, V],
            "tff_robust_pose_dev": [V, I32, V, I32, V, U64, I64, I32, F64, I32, I32, V, V, V, V, V, V],
            "tff_robust_pose_host": [V, I32, V, I32, V, U64, I64, I32, F64, I32, I32, V, V, V, V, V, V],
            "tff_robust_pose_scenes_dev": [V, I32, V, V, I64, I32, I64, V, I64, U64, I64, I32, F64, I32, I32, V, V, V, V, V, V],
            "tff_robust_pose_scenes_host": [V, I32, V, V, I64, V, I64, U64, I64, I32, F64, I32, I32, V, V, V, V, V, V],
            "tff_inlier_count_scenes_dev": [V, V, V, I64, I64, V, I64, V, V, I64, F64, V],
            "tff_robust_pose_scenes_adaptive_dev": [V, I32, V, V, I64, I32, I64, V, I64, U64, I64, I32, F64, I32, I32, F64, I32, V, V, V, V, V, V, V],
            "tff_robust_pose_scenes_adaptive_host": [V, I32, V, V, I64, V, I64, U64, I64, I32, F64, I32, I32, F64, I32, V, V, V, V, V, V, V],
            "tff_robust_round_plan": [F64, I64, I32, V, V, V],
            "tff_robust_pose_scenes_guided_dev": [V, I32, V, V, I64, I32, I64, V, I64, U64, I64, I32, F64, I32, I32, F64, I32, V, I64, V, V, V, V, V, V, V],
            "tff_robust_pose_scenes_guided_host": [V, I32, V, V, I64, V, I64, U64, I64, I32, F64, I32, I32, F64, I32, V, I64, V, V, V, V, V, V, V],
            "tff_sample_indices_guided_dev": [V, U64, I64, I64, I32, I32, V, I64, V],
            "tff_bundle_adjust_ragged_dev": [V, V, V, I64, V, V, I64, V, V, V, I64, V, V, V, V, V, V, V],
            "tff_bundle_adjust_ragged_host": [V, V, V, V, V, I64, V, V, V, I64, V, V, V, V, V, V, V],
            "tff_bundle_adjust_ragged_class_bounds": [V],
            "tff_optim_f_ragged_bounds": [V],
            "tff_bundle_adjust_loss_batch_dev": [V, V, I64, V, V, V, I64, I32, V, V, V, V, V, V, V, I32, F64, V],
            "tff_bundle_adjust_loss_batch_host": [V, V, I64, V, V, V, I64, I32, V, V, V, V, V, V, V, I32, F64, V],
            "tff_bundle_adjust_loss_ragged_dev": [V, V, V, I64, V, V, I64, V, V, V, I64, V, V, V, V, V, V, V, I32, F64, V],
            "tff_bundle_adjust_loss_ragged_host": [V, V, V, V, V, I64, V, V, V, I64, V, V, V, V, V, V, V, I32, F64, V],
            "tff_ba_covariance_batch_dev": [V, V, I64, V, V, V, I64, I32, V, I32, F64, V, V, V],
            "tff_ba_covariance_batch_host": [V, V, I64, V, V, V, I64, I32, V, I32, F64, V, V, V],
            "tff_ba_covariance_ragged_dev": [V, V, V, I64, V, V, I64, V, V, V, I64, I32, F64, V, V, V],
            "tff_ba_covariance_ragged_host": [V, V, V, V, V, I64, V, V, V, I64, I32, F64, V, V, V],
            "tff_bundle_adjust_cov_batch_dev": [V, V, I64, V, V, V, I64, I32, V, V, V, V, V, V, V, I32, F64, V, V, V, V],
            "tff_bundle_adjust_cov_batch_host": [V, V, I64, V, V, V, I64, I32, V, V, V, V, V, V, V, I32, F64, V, V, V, V],
            "tff_bundle_adjust_cov_ragged_dev": [V, V, V, I64, V, V, I64, V, V, V, I64, V, V, V, V, V, V, V, I32, F64, V, V, V, V],
            "tff_bundle_adjust_cov_ragged_host": [V, V, V, V, V, I64, V, V, V, I64, V, V, V, V, V, V, V, I32, F64, V, V, V, V],
            "tff_bundle_adjust_tracks_batch_dev": [V, I32, V, I64, V, V, I64, I32, V, V, V, V, V, V, V],
            "tff_bundle_adjust_tracks_batch_host": [V, I32, V, I64, V, V, I64, I32, V, V, V, V, V, V, V],
            "tff_bundle_adjust_tracks_loss_batch_dev": [V, I32, V, I64, V, V, I64, I32, V, V, V, V, V, V, V, I32, F64, V],
            "tff_bundle_adjust_tracks_loss_batch_host": [V, I32, V, I64, V, V, I64, I32, V, V, V, V, V, V, V, I32, F64, V],
            "tff_ba_tracks_covariance_batch_dev": [V, I32, V, I64, V, V, I64, I32, V, I32, F64, V, V, V],
            "tff_ba_tracks_covariance_batch_host": [V, I32, V, I64, V, V, I64, I32, V, I32, F64, V, V, V],
            "tff_bundle_adjust_tracks_cov_batch_dev": [V, I32, V, I64, V, V, I64, I32, V, V, V, V, V, V, V, I32, F64, V, V, V, V],
            "tff_bundle_adjust_tracks_cov_batch_host": [V, I32, V, I64, V, V, I64, I32, V, V, V, V, V, V, V, I32, F64, V, V, V, V],
        }
        for name, sig in protos.items():
            if path is not None and name in ADAPTIVE_SYMBOLS + GUIDED_SYMBOLS + LOSS_SYMBOLS + COV_SYMBOLS + TRACKS_SYMBOLS + TRACKS_LOSS_SYMBOLS + TRACKS_COV_SYMBOLS and not hasattr(lib, name):
                continue                                                     # (an older build, loaded by its path next to this one for a comparison)
            fn = getattr(lib, name)
            fn.argtypes = sig
            fn.restype = ctypes.c_int
        lib.tff_multi_destroy.argtypes = [V]; lib.tff_multi_destroy.restype = None
        lib.tff_multi_size.argtypes = [V]; lib.tff_multi_size.restype = I32
        lib.tff_multi_ctx.argtypes = [V, I32]; lib.tff_multi_ctx.restype = V
        lib.tff_multi_shard.argtypes = [V, I64, I32, ctypes.POINTER(I64), ctypes.POINTER(I64)]; lib.tff_multi_shard.restype = None
        if path is None:
            _lib = lib
        return lib


# reference method name -> C entry point stem
POSE_METHODS = {
    "LinearTFTPoseEstimation": "tff_linear_tft_pose_batch",
    "LinearFPoseEstimation": "tff_linear_f_pose_batch",
    "ResslTFTPoseEstimation": "tff_ressl_tft_pose_batch",
    "FaugPapaTFTPoseEstimation": "tff_faugpapa_tft_pose_batch",
    "NordbergTFTPoseEstimation": "tff_nordberg_tft_pose_batch",
    "OptimFPoseEstimation": "tff_optim_f_pose_batch",
    "PiPoseEstimation": "tff_pi_pose_batch",
    "PiColPoseEstimation": "tff_picol_pose_batch",
}

# every symbol include/tftfund.h declares (checked by the CPU test-suite)
EXPORTED_SYMBOLS = [
    "tff_version", "tff_last_error", "tff_ctx_create", "tff_ctx_destroy", "tff_ctx_set_stream",
    "tff_ctx_use_own_stream", "tff_ctx_get_stream", "tff_ctx_set_option", "tff_ctx_synchronize",
    "tff_linear_tft_pose_batch_dev", "tff_linear_tft_pose_batch_host", "tff_linear_tft_pose_batch_debug_dev", "tff_linear_f_pose_batch_debug_dev",
    "tff_linear_f_pose_batch_dev", "tff_linear_f_pose_batch_host",
    "tff_ressl_tft_pose_batch_dev", "tff_ressl_tft_pose_batch_host", "tff_ressl_tft_pose_batch_debug_dev",
    "tff_faugpapa_tft_pose_batch_dev", "tff_faugpapa_tft_pose_batch_host", "tff_faugpapa_tft_pose_batch_debug_dev",
    "tff_nordberg_tft_pose_batch_dev", "tff_nordberg_tft_pose_batch_host", "tff_nordberg_tft_pose_batch_debug_dev",
    "tff_optim_f_pose_batch_dev", "tff_optim_f_pose_batch_host",
    "tff_pi_pose_batch_dev", "tff_pi_pose_batch_host", "tff_picol_pose_batch_dev", "tff_picol_pose_batch_host",
    "tff_pi_pose_batch_debug_dev",
    "tff_triangulate_batch_dev", "tff_repr_error_batch_dev", "tff_inlier_count_batch_dev", "tff_transform_tft_batch_dev",
    "tff_rt_from_tft_batch_dev", "tff_linear_tft_batch_dev", "tff_linear_f_batch_dev", "tff_bundle_adjust_batch_dev", "tff_bundle_adjust_batch_host", "tff_bundle_adjust_views_batch_dev", "tff_bundle_adjust_views_batch_host", "tff_linear_tft_pose_sampled_dev", "tff_linear_f_pose_sampled_dev",
    "tff_multi_create", "tff_multi_destroy", "tff_multi_size", "tff_multi_ctx", "tff_multi_shard", "tff_pose_batch_host_multi", "tff_pose_batch_dev_multi",
    "tff_pose_batch_ragged_dev", "tff_pose_batch_ragged_host",
    "tff_sample_indices_dev", "tff_inlier_mask_batch_dev", "tff_robust_pose_dev", "tff_robust_pose_host",
    "tff_robust_pose_scenes_dev", "tff_robust_pose_scenes_host", "tff_inlier_count_scenes_dev",
    "tff_bundle_adjust_ragged_dev", "tff_bundle_adjust_ragged_host", "tff_bundle_adjust_ragged_class_bounds",
    "tff_optim_f_ragged_bounds",
]
# ... and every symbol include/tftfund_adaptive.h declares: the entry points added after library version 103, in the header that tftfund.h includes at
# its end.  (EXPORTED_SYMBOLS is the ABI of version 103 and is pinned as such: tests/test_score_cpu.py, tests/test_capi_symbols.py.)
ADAPTIVE_SYMBOLS = ["tff_robust_pose_scenes_adaptive_dev", "tff_robust_pose_scenes_adaptive_host", "tff_robust_round_plan"]
# ... and every symbol include/tftfund_guided.h declares: the entry points added after library version 104 (quality-guided sampling)
GUIDED_SYMBOLS = ["tff_robust_pose_scenes_guided_dev", "tff_robust_pose_scenes_guided_host", "tff_sample_indices_guided_dev"]
# ... and every symbol include/tftfund_loss.h declares: the entry points added after library version 105 (robust losses in the bundle adjustment)
LOSS_SYMBOLS = ["tff_bundle_adjust_loss_batch_dev", "tff_bundle_adjust_loss_batch_host", "tff_bundle_adjust_loss_ragged_dev",
                "tff_bundle_adjust_loss_ragged_host"]
LOSS_IDS = {"huber": 1, "cauchy": 2}      # include/tftfund_loss.h TFF_LOSS_*; 0 is TFF_LOSS_NONE
# ... and every symbol include/tftfund_cov.h declares: the entry points added after library version 106 (covariances of the bundle adjustment)
COV_SYMBOLS = ["tff_ba_covariance_batch_dev", "tff_ba_covariance_batch_host", "tff_ba_covariance_ragged_dev", "tff_ba_covariance_ragged_host",
               "tff_bundle_adjust_cov_batch_dev", "tff_bundle_adjust_cov_batch_host", "tff_bundle_adjust_cov_ragged_dev", "tff_bundle_adjust_cov_ragged_host"]
# ... and every symbol include/tftfund_tracks.h declares: the entry points added after library version 107 (bundle adjustment with per-point visibility)
TRACKS_SYMBOLS = ["tff_bundle_adjust_tracks_batch_dev", "tff_bundle_adjust_tracks_batch_host"]
# ... and every symbol include/tftfund_tracks_loss.h declares: the entry points added after library version 108 (robust losses over tracks)
TRACKS_LOSS_SYMBOLS = ["tff_bundle_adjust_tracks_loss_batch_dev", "tff_bundle_adjust_tracks_loss_batch_host"]
# ... and every symbol include/tftfund_tracks_cov.h declares: the entry points added after library version 109 (covariances over tracks)
TRACKS_COV_SYMBOLS = ["tff_ba_tracks_covariance_batch_dev", "tff_ba_tracks_covariance_batch_host", "tff_bundle_adjust_tracks_cov_batch_dev",
                      "tff_bundle_adjust_tracks_cov_batch_host"]

# method ids of the multi-GPU entry points (include/tftfund.h TFF_METHOD_*: the order of experiments.m:51-59)
METHOD_IDS = {"LinearTFTPoseEstimation": 0, "ResslTFTPoseEstimation": 1, "NordbergTFTPoseEstimation": 2, "FaugPapaTFTPoseEstimation": 3,
              "PiPoseEstimation": 4, "PiColPoseEstimation": 5, "LinearFPoseEstimation": 6, "OptimFPoseEstimation": 7}


# methods a ragged call (Context.pose_batch_ragged) supports
RAGGED_METHODS = ("LinearTFTPoseEstimation", "LinearFPoseEstimation", "OptimFPoseEstimation")


# methods the robust estimator (Context.robust_pose) draws its hypotheses and refits with, and their minimal sample
ROBUST_METHODS = {"LinearTFTPoseEstimation": 7, "LinearFPoseEstimation": 8}


MAX_ROUNDS = 32              # rounds of the adaptive robust call (tff_robust_round_plan)
GUIDED_MAX_GROWTH = 2 ** 31 - 2 ** 25   # the largest `growth` of the guided sampler: its pool table stays an int32 (include/tftfund_guided.h)
GUIDED_MAX_N = 1 << 24       # ... for scenes of up to 2^24 correspondences, the bound of every robust call


# the entry point of Context.robust_pose_scenes (without its _host / _dev), by (ranking given, confidence given)
_ROBUST_SCENES_ENTRY = {(False, False): "tff_robust_pose_scenes", (False, True): "tff_robust_pose_scenes_adaptive",
                        (True, False): "tff_robust_pose_scenes_guided", (True, True): "tff_robust_pose_scenes_guided"}


def _np_ptr(a):
    """the pointer function of the _host forms (Context._p is that of the _dev forms); None is the null pointer"""
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _check_adaptive(confidence, first_round):
    """the adaptive arguments of robust_pose / robust_pose_scenes, refused as the library refuses them"""
    c = float(confidence)
    if not (0.0 < c < 1.0):
        raise ValueError("confidence must lie strictly between 0 and 1, not %r" % (confidence,))
    f = int(first_round)
    if f != first_round or f < 4 or f % 4 != 0 or f > 0x7FFFFFFC:
        raise ValueError("first_round must be a multiple of 4 and at least 4, not %r" % (first_round,))
    return c, f


def round_plan(confidence, n_hyp, first_round=256):
    """tff_robust_round_plan: (ends (R,) int64, qmin (R,) float64) of the adaptive robust call -- round r ends at ends[r - 1] =
    min(n_hyp, first_round << (r - 1)) hypotheses per scene, where a scene stops once adaptive_stop(...) holds at qmin[r - 1] =
    -expm1(log1p(-confidence) / ends[r - 1]).  Needs no context and no GPU."""
    c, f = _check_adaptive(confidence, first_round)
    if int(n_hyp) != n_hyp or int(n_hyp) < 1:
        raise ValueError("n_hyp must be an integer of at least 1")
    lib = load_library()
    ends = np.zeros(MAX_ROUNDS, dtype=np.int64); qmin = np.zeros(MAX_ROUNDS); rounds = ctypes.c_int32(0)
    _check(lib, lib.tff_robust_round_plan(c, int(n_hyp), f, ctypes.c_void_p(ends.ctypes.data), ctypes.c_void_p(qmin.ctypes.data),
                                          ctypes.cast(ctypes.byref(rounds), ctypes.c_void_p)), "tff_robust_round_plan")
    return ends[:rounds.value].copy(), qmin[:rounds.value].copy()


def adaptive_stop(best, ns, n_sample, qmin, msac=False):
    """The stop rule of the adaptive robust call in numpy, decision for decision what the device computes: best = the largest count (score with msac)
    of the scene so far (-1: no success), ns its correspondences.  I = best (// SCORE_UNITS with msac); stop iff I >= 1 and (I / ns) multiplied by
    itself n_sample - 1 times, in double, is >= qmin."""
    I = int(best) // SCORE_UNITS if (msac and best >= 0) else int(best)
    if I < 1:
        return False
    w = np.float64(I) / np.float64(ns)
    q = w
    for _ in range(int(n_sample) - 1):
        q = q * w
    return bool(q >= np.float64(qmin))


def _check_loss(loss, scale, what="loss", default_scale=None):
    """the robust loss of a bundle adjustment: None (and then no scale), or "huber" / "cauchy" with a positive finite scale in pixels
    -> None or (TFF_LOSS_* id, scale)"""
    if loss is None:
        if scale is not None:
            raise ValueError("a %s scale without a loss" % what)
        return None
    if loss not in LOSS_IDS:
        raise ValueError("%s must be None, 'huber' or 'cauchy', not %r" % (what, loss))
    if scale is None:
        scale = default_scale
    if isinstance(scale, bool) or not isinstance(scale, (int, float, np.integer, np.floating)) or not (scale > 0 and np.isfinite(scale)):
        raise ValueError("the scale of the %s must be a positive finite number of pixels, not %r" % (what, scale))
    return LOSS_IDS[loss], float(scale)


def _splitmix64(x):
    z = x + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _sample_rows(seed, h, n, Ns):
    """the sampler of sample_indices_reference for rows with their own hypothesis index h (uint64) and their own Ns (a scalar or one per row): (len(h), n)
    int64.  A Fisher-Yates shuffle of the virtual array 0 .. Ns-1 of which only the n swaps are kept; wrapping uint64."""
    B = h.shape[0]
    Ns = np.broadcast_to(np.asarray(Ns, dtype=np.int64), (B,))
    with np.errstate(over="ignore"):
        key = _splitmix64(np.uint64(seed) ^ (h * np.uint64(0xD1342543DE82EF95)))
        out = np.empty((B, n), dtype=np.int64)
        pos = np.empty((B, n), dtype=np.int64)
        val = np.empty((B, n), dtype=np.int64)

        def look(p, m):                      # the value of the LAST of the first m records whose position is p, else p
            v = p.copy()
            for j in range(m):
                v = np.where(pos[:, j] == p, val[:, j], v)
            return v

        for i in range(n):
            u = _splitmix64(key + np.uint64(i)) >> np.uint64(32)
            r = (np.uint64(i) + ((u * (Ns - i).astype(np.uint64)) >> np.uint64(32))).astype(np.int64)
            vr, vi = look(r, i), look(np.full(B, i, dtype=np.int64), i)
            out[:, i] = vr
            pos[:, i] = r
            val[:, i] = vi
    return out


def sample_indices_reference(seed, first, B, n, Ns):
    """What tff_sample_indices_dev computes (include/tftfund.h), in numpy: (B, n) int32, row b = n distinct indices in [0, Ns), a function of
    (seed, first + b, n, Ns) only.  A Fisher-Yates shuffle of the virtual array 0 .. Ns-1 of which only the n swaps are kept; wrapping uint64."""
    if not (1 <= n <= 16 and Ns >= n and B >= 0 and first >= 0):
        raise ValueError("need 1 <= n <= 16, Ns >= n, B >= 0, first >= 0")
    with np.errstate(over="ignore"):
        h = np.uint64(first) + np.arange(B, dtype=np.uint64)
    return _sample_rows(seed, h, n, Ns).astype(np.int32)


def _check_growth(growth):
    """the growth of the guided sampler, refused as the library refuses it"""
    g = int(growth)
    if g != growth or not (1 <= g <= GUIDED_MAX_GROWTH):
        raise ValueError("growth must be an integer between 1 and 2^31 - 2^25, not %r" % (growth,))
    return g


def guided_pool_ends(Ns, n, growth):
    """The pool table of the guided (PROSAC) sampler for a scene of Ns correspondences and samples of n (include/tftfund_guided.h), in numpy: (Ns + 1,)
    int32 with ends[k] = 0 below n, ends[n] = 1 and ends[k + 1] = ends[k] + ceil(T(k + 1) - T(k)), T(k) = growth * C(k, n) / C(Ns, n) evaluated in double
    as growth * (k - i) / (Ns - i) over i = 0 .. n-1, multiply then divide.  The 1-based hypothesis t draws from the smallest pool k with ends[k] >= t,
    uniformly beyond ends[Ns] (<= growth + Ns)."""
    G = _check_growth(growth)
    Ns, n = int(Ns), int(n)
    if not (1 <= n <= 16 and n <= Ns <= GUIDED_MAX_N):
        raise ValueError("need 1 <= n <= 16 and n <= Ns <= 2^24")
    k = np.arange(n, Ns + 1, dtype=np.float64)
    T = np.full(k.shape, np.float64(G))
    for i in range(n):
        T = T * (k - np.float64(i))
        T = T / np.float64(Ns - i)
    ends = np.zeros(Ns + 1, dtype=np.int64)
    ends[n] = 1
    ends[n + 1:] = 1 + np.cumsum(np.ceil(T[1:] - T[:-1]).astype(np.int64))
    return ends.astype(np.int32)


def guided_pool(ends, n, t):
    """the pool of the 1-based hypotheses t (array) under the table `ends` of guided_pool_ends: the smallest k in [n, Ns] with ends[k] >= t, 0 where
    t > ends[Ns] (the uniform draw)"""
    t = np.asarray(t, dtype=np.uint64)
    pool = n + np.searchsorted(ends[n:].astype(np.uint64), t, side="left")
    return np.where(t > np.uint64(ends[-1]), 0, pool).astype(np.int64)


def sample_indices_guided_reference(seed, first, B, n, order, growth):
    """What tff_sample_indices_guided_dev computes (include/tftfund_guided.h), in numpy: (B, n) int32.  order (Ns,) is the scene's ranking, best first.
    Hypothesis h = first + b with the pool k = guided_pool(ends, n, h + 1) draws the n - 1 ranks of the uniform sampler for (seed, h, n - 1, k - 1) and
    then rank k - 1; without a pool the uniform sampler's ranks for (seed, h, n, Ns).  Row = order[ranks], or all -1 if one of those entries lies outside
    [0, Ns)."""
    order = np.asarray(order)
    if order.ndim != 1 or not np.issubdtype(order.dtype, np.integer):
        raise ValueError("order must be a 1-D integer array")
    Ns = order.shape[0]
    if not (B >= 0 and first >= 0):
        raise ValueError("need B >= 0, first >= 0")
    ends = guided_pool_ends(Ns, n, growth)
    with np.errstate(over="ignore"):
        h = np.uint64(first) + np.arange(B, dtype=np.uint64)
        pool = guided_pool(ends, n, h + np.uint64(1))
    ranks = np.empty((B, n), dtype=np.int64)
    uni = pool == 0
    ranks[uni] = _sample_rows(seed, h[uni], n, Ns)
    if n > 1:
        ranks[~uni, :n - 1] = _sample_rows(seed, h[~uni], n - 1, pool[~uni] - 1)
    ranks[~uni, n - 1] = pool[~uni] - 1
    idx = order.astype(np.int64)[ranks]
    bad = ((idx < 0) | (idx >= Ns)).any(axis=1)
    idx[bad] = -1
    return idx.astype(np.int32)


def order_from_quality(quality, offsets):
    """The ranking the robust calls build from quality= on the host: quality (Ntot,) float, higher is better, NaN last; offsets (S + 1,) int64.  A stable
    sort by descending quality, then a stable sort by scene, minus the scene's first offset: (Ntot,) int32, the ranking of scene s at offsets[s].  A packed
    entry in front of offsets[0] or behind offsets[S] belongs to no scene: it keeps a slot outside every scene's range, which holds -1."""
    q = np.asarray(quality, dtype=np.float64)
    off = np.asarray(offsets, dtype=np.int64)
    q = np.where(np.isnan(q), -np.inf, q)
    by_q = np.argsort(-q, kind="stable")
    S = off.shape[0] - 1
    scene = np.searchsorted(off, np.arange(q.shape[0], dtype=np.int64), side="right") - 1     # -1 in front of offsets[0], S behind offsets[S]
    glob = by_q[np.argsort(scene[by_q], kind="stable")]
    sg = scene[glob]
    return np.where((sg >= 0) & (sg < S), glob - off[np.clip(sg, 0, S)], -1).astype(np.int32)


def euler_cov_to_rotvec(R_t_2, R_t_3, cov):
    """The covariance of a bundle adjustment (bundle_adjust(..., cov=True), ba_covariance: parameters angles2, angles3, t2, t3 with the angles of
    R = Rx(a) Ry(b) Rz(c), BundleAdjustment.m:92-94) in LEFT-PERTURBATION ROTATION-VECTOR coordinates: parameters omega2, omega3, t2, t3 with
    R(angles + d) = exp([omega]x) R(angles) to first order, omega = e_x da + Rx e_y db + Rx Ry e_z dc.  sqrt of the trace of a 3 x 3 rotation block is
    then the rotation's standard deviation in radians, whatever the angles are.  Host helper, numpy: R_t_2, R_t_3 (3,4) or (B,3,4), cov (12,12) or
    (B,12,12) -> the same shape."""
    to_np = lambda a: np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
    r2, r3, cv = to_np(R_t_2), to_np(R_t_3), to_np(cov)
    single = cv.ndim == 2
    if single:
        r2, r3, cv = r2[None], r3[None], cv[None]
    if r2.shape[1:] != (3, 4) or r3.shape != r2.shape or cv.shape != (r2.shape[0], 12, 12):
        raise ValueError("R_t_2, R_t_3 must be (B, 3, 4) and cov (B, 12, 12)")
    out = np.empty_like(cv)
    for b in range(cv.shape[0]):
        T = np.eye(12)
        for j, R in enumerate((r2[b][:, :3], r3[b][:, :3])):
            a = -np.arctan2(R[1, 2], R[2, 2]); bb = -np.arctan2(-R[0, 2], np.hypot(R[1, 2], R[2, 2]))
            ca, sa, cb, sb = np.cos(a), np.sin(a), np.cos(bb), np.sin(bb)
            Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]]); Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
            T[3 * j:3 * j + 3, 3 * j:3 * j + 3] = np.stack([np.array([1.0, 0, 0]), Rx[:, 1], (Rx @ Ry)[:, 2]], axis=1)
        out[b] = T @ cv[b] @ T.T
    return out[0] if single else out


def euler_cov_to_rotvec_views(R_t, cov):
    """euler_cov_to_rotvec for the M - 1 cameras of a bundle adjustment over tracks (bundle_adjust_views(..., missing="point", cov=True),
    ba_tracks_covariance: parameters angles of cameras 2..M, then their translations): the same first-order map to LEFT-PERTURBATION ROTATION-VECTOR
    coordinates, omega_j = e_x da + Rx e_y db + Rx Ry e_z dc per camera; the translations pass through.  Host helper, numpy: R_t (3M,4) or (B,3M,4),
    cov (P,P) or (B,P,P) with P = 6 (M - 1) -> the same shape."""
    to_np = lambda a: np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
    rt, cv = to_np(R_t), to_np(cov)
    single = cv.ndim == 2
    if single:
        rt, cv = rt[None], cv[None]
    if rt.ndim != 3 or rt.shape[2] != 4 or rt.shape[1] % 3 or not 2 <= rt.shape[1] // 3 <= 6 or cv.shape != (rt.shape[0],) + (6 * (rt.shape[1] // 3 - 1),) * 2:
        raise ValueError("R_t must be (B, 3M, 4) with M = 2 .. 6 and cov (B, 6 (M - 1), 6 (M - 1))")
    C = rt.shape[1] // 3 - 1
    out = np.empty_like(cv)
    for b in range(cv.shape[0]):
        T = np.eye(6 * C)
        for j in range(C):
            R = rt[b][3 * j + 3:3 * j + 6, :3]
            a = -np.arctan2(R[1, 2], R[2, 2]); bb = -np.arctan2(-R[0, 2], np.hypot(R[1, 2], R[2, 2]))
            ca, sa, cb, sb = np.cos(a), np.sin(a), np.cos(bb), np.sin(bb)
            Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]]); Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
            T[3 * j:3 * j + 3, 3 * j:3 * j + 3] = np.stack([np.array([1.0, 0, 0]), Rx[:, 1], (Rx @ Ry)[:, 2]], axis=1)
        out[b] = T @ cv[b] @ T.T
    return out[0] if single else out


def pack_ragged(items):
    """A list of (n_b, 6) correspondence arrays (n_b may differ, and be 0) -> (corresp (sum n_b, 6) float64, offsets (B + 1,) int64):
    the packed layout of the ragged entry points, triplet b = corresp[offsets[b]:offsets[b + 1]]."""
    arrs = []
    for k, a in enumerate(items):
        a = np.asarray(a, dtype=np.float64)
        if a.ndim != 2 or (a.shape[1] != 6 and a.size):
            raise ValueError("item %d: correspondences must be (n, 6)" % k)
        arrs.append(a.reshape(-1, 6))
    offsets = np.zeros(len(arrs) + 1, dtype=np.int64)
    if arrs:
        offsets[1:] = np.cumsum([a.shape[0] for a in arrs])
    corresp = np.concatenate(arrs, axis=0) if arrs else np.zeros((0, 6))
    return np.ascontiguousarray(corresp), offsets


def check_offsets(offsets):
    """Validate a host offsets array (B + 1 int64, offsets[0] >= 0, non-decreasing); returns n_max (0 for an empty batch)."""
    offsets = np.asarray(offsets)
    if offsets.ndim != 1 or offsets.shape[0] < 1:
        raise ValueError("offsets must be a 1-D array of B + 1 entries")
    if not np.issubdtype(offsets.dtype, np.integer):
        raise ValueError("offsets must be integers")
    if offsets[0] < 0:
        raise ValueError("offsets[0] must be >= 0")
    n = np.diff(offsets.astype(np.int64))
    if n.size and n.min() < 0:
        raise ValueError("offsets must not decrease (item %d)" % int(np.argmin(n)))
    return int(n.max()) if n.size else 0


def ba_ragged_class_bounds():
    """tff_bundle_adjust_ragged_class_bounds: the largest number of selected correspondences of each of the three launch classes of
    Context.bundle_adjust_ragged (LDS per item up to 40, 80, 160 KiB); the last one is BA_MAX_N."""
    lib = load_library()
    b = (ctypes.c_int32 * 3)()
    _check(lib, lib.tff_bundle_adjust_ragged_class_bounds(b), "tff_bundle_adjust_ragged_class_bounds")
    return tuple(int(v) for v in b)


def optim_f_ragged_bounds():
    """tff_optim_f_ragged_bounds: (S, L), the largest correspondence counts at which the Gauss-Helmert refinement of OptimFPoseEstimation keeps the
    normalised observations in LDS (S) and its estimates in LDS under the default options (L): the boundaries of the three launch classes of
    Context.pose_batch_ragged("OptimFPoseEstimation", ...), and of the fixed-N call's storage routes."""
    lib = load_library()
    b = (ctypes.c_int32 * 2)()
    _check(lib, lib.tff_optim_f_ragged_bounds(b), "tff_optim_f_ragged_bounds")
    return tuple(int(v) for v in b)


def _check(lib, rc, what):
    if rc != 0:
        msg = lib.tff_last_error()
        raise TffError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else "?"))


class Context:
    """A tff_ctx: one device, one stream.  `solver`: 'invit' (fast tiers -- Gram matrix + Cholesky inverse iteration,
    certified sign-only votes -- with the exact kernel over what they cannot finish) or 'exact' (exact kernel for every
    triplet: Householder QR of the explicit design matrix, one-sided Jacobi fall-backs; 'jacobi' is the old name)."""

    def __init__(self, device=0, solver="invit", stage_lds=-1, lib_path=None):
        self.lib = load_library(lib_path)
        h = ctypes.c_void_p()
        _check(self.lib, self.lib.tff_ctx_create(ctypes.byref(h), int(device)), "tff_ctx_create")
        self.handle = h
        self.device = int(device)
        self.set_solver(solver)
        _check(self.lib, self.lib.tff_ctx_set_option(self.handle, TFF_OPT_STAGE_LDS, int(stage_lds)), "set_option")

    def set_solver(self, solver):
        v = {"invit": 0, "jacobi": 1, "exact": 1}[solver]
        _check(self.lib, self.lib.tff_ctx_set_option(self.handle, TFF_OPT_SOLVER, v), "set_option")

    def set_exact_below(self, n):
        """TFF_OPT_EXACT_BELOW: batches with fewer than n correspondences per triplet go to the exact kernel as a whole
        (default 12); 0 = only the triplets the fast tiers flag."""
        _check(self.lib, self.lib.tff_ctx_set_option(self.handle, TFF_OPT_EXACT_BELOW, int(n)), "set_option")

    def set_spill_only_if_needed(self, on):
        """TFF_OPT_SPILL: True = the per-correspondence state of the iterative methods stays in LDS whenever it fits (fewer workgroups per CU,
        HBM traffic near the algorithmic bytes); False (default) = it goes to global slices when that raises the occupancy."""
        _check(self.lib, self.lib.tff_ctx_set_option(self.handle, TFF_OPT_SPILL, int(bool(on))), "set_option")

    def set_count_rows(self, on):
        """TFF_OPT_COUNT_ROWS: inlier counts with four hypotheses per wavefront (default) or one."""
        _check(self.lib, self.lib.tff_ctx_set_option(self.handle, TFF_OPT_COUNT_ROWS, int(bool(on))), "set_option")

    def set_score(self, score):
        """TFF_OPT_SCORE: "count" (default) = inlier_count / inlier_count_scenes return inlier counts and robust_pose / robust_pose_scenes rank their
        hypotheses, adopt refits and pick the winner by them; "msac" = by the MSAC score instead, an int32 sum of per-inlier weights
        1 + int(63 max(0, 1 - ss / (6 threshold^2))), ss the sum of the inlier's six squared residuals (include/tftfund.h).  inlier_mask, the returned
        mask and `inliers` stay hard counts; with "msac" the robust estimators add out["score"], the score of the returned pose (-1: no pose)."""
        if score not in SCORES:
            raise ValueError("score must be one of %s, not %r" % (", ".join(map(repr, SCORES)), score))
        _check(self.lib, self.lib.tff_ctx_set_option(self.handle, TFF_OPT_SCORE, SCORES[score]), "set_option")
        self._score = SCORES[score]

    def set_ba_classes(self, mode):
        """TFF_OPT_BA_CLASSES: how bundle_adjust_ragged launches its items.  "auto" / 0 (default) = one launch sized for BA_MAX_N up to 256 items, three
        launch classes by LDS need beyond; 1 = one launch always; 2 = three classes always (A/B switch).  Identical results."""
        _check(self.lib, self.lib.tff_ctx_set_option(self.handle, TFF_OPT_BA_CLASSES, 0 if mode == "auto" else int(mode)), "set_option")

    def set_rows(self, on):
        """TFF_OPT_ROWS: "auto" / 2 (default) and True / 1 = the row kernels (four triplets per wavefront, one per row of 16 lanes) at any batch size:
        a triplet's bits do not depend on the batch it arrives in; False / 0 = one triplet per wavefront (lowest latency for small batches)."""
        v = 2 if on == "auto" else (int(on) if isinstance(on, int) and not isinstance(on, bool) else int(bool(on)))
        _check(self.lib, self.lib.tff_ctx_set_option(self.handle, TFF_OPT_ROWS, v), "set_option")

    def set_pre(self, on):
        """TFF_OPT_PRE (A/B switch): False / 0 (default) = normalisations + moment sums inside the trifocal row kernels; True / 1 = in a kernel of
        their own (one triplet per wavefront, correspondences read once; measured slower: profiles/r5_ab_pre.txt); "auto" / 2 = that kernel from N >= 48."""
        v = 2 if on == "auto" else (int(on) if isinstance(on, int) and not isinstance(on, bool) else int(bool(on)))
        _check(self.lib, self.lib.tff_ctx_set_option(self.handle, TFF_OPT_PRE, v), "set_option")

    def set_debug_adaptive(self, on):
        """TFF_OPT_DEBUG_ADAPTIVE (profiling hook): debug entry points keep the production cheirality-vote logic."""
        _check(self.lib, self.lib.tff_ctx_set_option(self.handle, TFF_OPT_DEBUG_ADAPTIVE, int(bool(on))), "set_option")

    def set_debug_fp_handover(self, on):
        """TFF_OPT_DEBUG_FP_HANDOVER (test hook): FaugPapa's block kernel hands every third triplet back to the generic workgroup kernel."""
        _check(self.lib, self.lib.tff_ctx_set_option(self.handle, TFF_OPT_DEBUG_FP_HANDOVER, int(bool(on))), "set_option")

    def set_gh_exact(self, on):
        """Gauss-Helmert methods: True = pinv(W) always through per-block eigen-decompositions (A/B; slower)."""
        _check(self.lib, self.lib.tff_ctx_set_option(self.handle, TFF_OPT_GH_EXACT, int(bool(on))), "set_option")

    def set_kernel_variant(self, v):
        """TFF_OPT_KERNEL.  Iterative TFT methods:
        0 automatic (a workgroup per triplet at every N), 1 the fused single-wavefront kernels, 2 workgroup always (FaugPapa: the generic
        block kernel instead of its own)."""
        _check(self.lib, self.lib.tff_ctx_set_option(self.handle, TFF_OPT_KERNEL, int(v)), "set_option")

    def set_stream(self, stream_ptr):
        """Enqueue on the caller's hipStream_t (0 / None = the device's null stream, torch's default)."""
        _check(self.lib, self.lib.tff_ctx_set_stream(self.handle, ctypes.c_void_p(stream_ptr or 0)), "set_stream")

    def use_own_stream(self):
        _check(self.lib, self.lib.tff_ctx_use_own_stream(self.handle), "use_own_stream")

    def stream_ptr(self):
        """The hipStream_t the context launches on (its own stream unless set_stream was called), as an integer."""
        return int(self.lib.tff_ctx_get_stream(self.handle) or 0)

    def synchronize(self):
        _check(self.lib, self.lib.tff_ctx_synchronize(self.handle), "synchronize")

    def close(self):
        if getattr(self, "handle", None):
            self.lib.tff_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- batched pose estimation ------------------------------------------
    def pose_batch(self, method, corresp, calm, reconst=True, debug=False):
        """corresp: (B, N, 6) float64 (== MATLAB 6 x N x B); calm: (9,3) shared or
        (B, 9, 3).  numpy in -> numpy out (host path); torch CUDA tensors in ->
        torch tensors out (device path, asynchronous on the current stream).
        Returns dict(R_t_2 (B,3,4), R_t_3 (B,3,4), T (B,3,3,3) indexed [b,j,k,i],
        Reconst (B,3,N) or None, iter (B,), status (B,))."""
        stem = POSE_METHODS[method]
        if isinstance(corresp, np.ndarray):
            return self._pose_batch_host(stem, corresp, calm, reconst)
        return self._pose_batch_dev(stem, corresp, calm, reconst, debug)

    @staticmethod
    def _calm_cm_np(calm, B):
        calm = np.asarray(calm, dtype=np.float64)
        if calm.shape == (9, 3):
            return np.ascontiguousarray(calm.T).reshape(27), 0
        if calm.shape == (B, 9, 3):
            return np.ascontiguousarray(calm.transpose(0, 2, 1)).reshape(B * 27), 27
        raise ValueError("CalM must be 9x3 or Bx9x3")

    def _pose_batch_host(self, stem, corresp, calm, reconst):
        corresp = np.ascontiguousarray(corresp, dtype=np.float64)
        if corresp.ndim != 3 or corresp.shape[2] != 6:
            raise ValueError("corresp must be (B, N, 6)")
        B, N, _ = corresp.shape
        calm_cm, stride = self._calm_cm_np(calm, B)
        Rt2 = np.empty((B, 12)); Rt3 = np.empty((B, 12)); T = np.empty((B, 27))
        rec = np.empty((B, N, 3)) if reconst else None
        it = np.zeros(B, dtype=np.int32); st = np.zeros(B, dtype=np.int32)
        fn = getattr(self.lib, stem + "_host")
        ptr = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None
        _check(self.lib, fn(self.handle, ptr(corresp), ptr(calm_cm), stride, B, N, ptr(Rt2), ptr(Rt3), ptr(T), ptr(rec),
                            ptr(it), ptr(st)), stem + "_host")
        return dict(R_t_2=Rt2.reshape(B, 4, 3).transpose(0, 2, 1), R_t_3=Rt3.reshape(B, 4, 3).transpose(0, 2, 1),
                    T=T.reshape(B, 3, 3, 3).transpose(0, 3, 2, 1),
                    Reconst=rec.transpose(0, 2, 1) if reconst else None, iter=it, status=st)

    def _pose_batch_dev(self, stem, corresp, calm, reconst, debug):
        if not (corresp.is_cuda and corresp.dtype == torch.float64 and corresp.is_contiguous()):
            raise ValueError("corresp must be a contiguous float64 CUDA tensor of shape (B, N, 6)")
        B, N, _ = corresp.shape
        dev = corresp.device
        if tuple(calm.shape) == (9, 3):
            calm_cm, stride = calm.t().contiguous().reshape(27), 0
        elif tuple(calm.shape) == (27,):
            calm_cm, stride = calm.contiguous(), 0          # already column-major
        else:
            calm_cm, stride = calm.transpose(1, 2).contiguous().reshape(B * 27), 27
        calm_cm = calm_cm.to(device=dev, dtype=torch.float64)
        Rt2 = torch.empty((B, 12), dtype=torch.float64, device=dev)
        Rt3 = torch.empty((B, 12), dtype=torch.float64, device=dev)
        T = torch.empty((B, 27), dtype=torch.float64, device=dev)
        rec = torch.empty((B, N, 3), dtype=torch.float64, device=dev) if reconst else None
        it = torch.zeros(B, dtype=torch.int32, device=dev)
        st = torch.zeros(B, dtype=torch.int32, device=dev)
        self.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        out = dict()
        if debug and stem in ("tff_pi_pose_batch", "tff_picol_pose_batch"):
            # the start of the Gauss-Helmert iteration: `pi` (27) and `x_est` (6N) per triplet
            ip = torch.zeros((B, 27), dtype=torch.float64, device=dev)
            ix = torch.zeros((B, 6 * N), dtype=torch.float64, device=dev)
            _check(self.lib, self.lib.tff_pi_pose_batch_debug_dev(self.handle, int(stem == "tff_picol_pose_batch"), p(corresp), p(calm_cm), stride,
                                                                  B, N, p(Rt2), p(Rt3), p(T), p(rec), p(it), p(st), p(ip), p(ix)),
                   "tff_pi_pose_batch_debug_dev")
            out["init_p"] = ip
            out["init_x"] = ix
        elif debug:
            dbg = torch.zeros((B, DEBUG_STRIDE), dtype=torch.float64, device=dev)
            fn = getattr(self.lib, stem + "_debug_dev")
            _check(self.lib, fn(self.handle, p(corresp), p(calm_cm), stride, B, N, p(Rt2), p(Rt3), p(T), p(rec), p(it), p(st),
                                p(dbg)), stem + "_debug_dev")
            out["debug"] = dbg
        else:
            fn = getattr(self.lib, stem + "_dev")
            _check(self.lib, fn(self.handle, p(corresp), p(calm_cm), stride, B, N, p(Rt2), p(Rt3), p(T), p(rec), p(it), p(st)),
                   stem + "_dev")
        out.update(R_t_2=Rt2.reshape(B, 4, 3).transpose(1, 2), R_t_3=Rt3.reshape(B, 4, 3).transpose(1, 2),
                   T=T.reshape(B, 3, 3, 3).permute(0, 3, 2, 1),
                   Reconst=rec.transpose(1, 2) if reconst else None, iter=it, status=st,
                   _raw=(Rt2, Rt3, T, rec))
        return out


    def pose_batch_ragged(self, method, corresp, offsets, calm, reconst=True, n_max=None):
        """One call for triplets with different correspondence counts (LinearTFT, LinearF, OptimF): corresp (Ntot, 6) packed, offsets (B + 1,)
        int64 with triplet b = corresp[offsets[b]:offsets[b + 1]] (see pack_ragged); calm (9, 3) shared or (B, 9, 3).  Each triplet's
        outputs are bit-identical to pose_batch() on that triplet alone.  numpy in -> numpy out (host path; malformed offsets raise).
        torch CUDA tensors in (offsets on the same device) -> torch tensors out, asynchronous on the current stream; n_max bounds every
        n_b (a larger one marks the item ST_BAD_OFFSETS) -- pass it to avoid the one synchronisation that computes it from the offsets.
        Returns dict(R_t_2 (B,3,4), R_t_3 (B,3,4), T (B,3,3,3), Reconst (Ntot,3) packed or None, iter (B,), status (B,)); iter carries the
        Gauss-Helmert counts of OptimF (0 for the linear methods)."""
        if method not in METHOD_IDS:
            raise ValueError("unknown method %r" % (method,))
        mid = METHOD_IDS[method]
        if isinstance(corresp, np.ndarray):
            corresp = np.ascontiguousarray(corresp, dtype=np.float64).reshape(-1, 6)
            offsets = np.ascontiguousarray(offsets, dtype=np.int64)
            check_offsets(offsets)
            B = offsets.shape[0] - 1
            if offsets[-1] > corresp.shape[0]:
                raise ValueError("offsets[-1] = %d beyond the %d packed correspondences" % (offsets[-1], corresp.shape[0]))
            calm_cm, stride = self._calm_cm_np(calm, B)
            Rt2 = np.empty((B, 12)); Rt3 = np.empty((B, 12)); T = np.empty((B, 27))
            rec = np.full((corresp.shape[0], 3), np.nan) if reconst else None
            it = np.zeros(B, dtype=np.int32); st = np.zeros(B, dtype=np.int32)
            ptr = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None
            _check(self.lib, self.lib.tff_pose_batch_ragged_host(self.handle, mid, ptr(corresp), ptr(offsets), ptr(calm_cm), stride, B, ptr(Rt2),
                                                                 ptr(Rt3), ptr(T), ptr(rec), ptr(it), ptr(st)), "tff_pose_batch_ragged_host")
            return dict(R_t_2=Rt2.reshape(B, 4, 3).transpose(0, 2, 1), R_t_3=Rt3.reshape(B, 4, 3).transpose(0, 2, 1),
                        T=T.reshape(B, 3, 3, 3).transpose(0, 3, 2, 1), Reconst=rec, iter=it, status=st)
        if not (corresp.is_cuda and corresp.dtype == torch.float64 and corresp.is_contiguous()):
            raise ValueError("corresp must be a contiguous float64 CUDA tensor of shape (Ntot, 6)")
        dev = corresp.device
        if not (offsets.is_cuda and offsets.device == dev and offsets.dtype == torch.int64 and offsets.dim() == 1):
            raise ValueError("offsets must be a 1-D int64 tensor on the device of corresp")
        offsets = offsets.contiguous()
        B = offsets.shape[0] - 1
        if n_max is None:                                                   # one synchronisation; pass n_max to avoid it
            n_max = max(0, int((offsets[1:] - offsets[:-1]).max().item())) if B > 0 else 0   # (negative n_b: ST_BAD_OFFSETS per item)
        if isinstance(calm, np.ndarray):
            calm = torch.from_numpy(np.ascontiguousarray(calm, dtype=np.float64))
        if not isinstance(calm, torch.Tensor) or tuple(calm.shape) not in ((9, 3), (B, 9, 3)):
            raise ValueError("CalM must be a (9, 3) or (B, 9, 3) array or tensor")
        if tuple(calm.shape) == (9, 3):
            calm_cm, stride = calm.t().contiguous().reshape(27), 0
        else:
            calm_cm, stride = calm.transpose(1, 2).contiguous().reshape(B * 27), 27
        calm_cm = calm_cm.to(device=dev, dtype=torch.float64)
        Rt2 = torch.empty((B, 12), dtype=torch.float64, device=dev)
        Rt3 = torch.empty((B, 12), dtype=torch.float64, device=dev)
        T = torch.empty((B, 27), dtype=torch.float64, device=dev)
        rec = torch.full((corresp.shape[0], 3), float("nan"), dtype=torch.float64, device=dev) if reconst else None
        it = torch.zeros(B, dtype=torch.int32, device=dev)
        st = torch.zeros(B, dtype=torch.int32, device=dev)
        self.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        _check(self.lib, self.lib.tff_pose_batch_ragged_dev(self.handle, mid, p(corresp), p(offsets), int(n_max), p(calm_cm), stride, B, p(Rt2),
                                                            p(Rt3), p(T), p(rec), p(it), p(st)), "tff_pose_batch_ragged_dev")
        return dict(R_t_2=Rt2.reshape(B, 4, 3).transpose(1, 2), R_t_3=Rt3.reshape(B, 4, 3).transpose(1, 2),
                    T=T.reshape(B, 3, 3, 3).permute(0, 3, 2, 1), Reconst=rec, iter=it, status=st, _raw=(Rt2, Rt3, T, rec))

    # ---- building blocks (torch CUDA tensors or numpy arrays in; torch CUDA tensors out) ------------
    def _t(self, a, dtype=None):
        dtype = dtype or torch.float64
        if isinstance(a, np.ndarray):
            a = torch.from_numpy(np.ascontiguousarray(a))
        return a.to(device=torch.device("cuda", self.device), dtype=dtype).contiguous()

    def _begin(self):
        self.set_stream(torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream)

    @staticmethod
    def _p(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else None

    @staticmethod
    def _cams_cm(cams):
        """(..., 3, 4) row-major numpy/torch cameras -> column-major flat layout of the ABI."""
        return cams.transpose(-1, -2).contiguous()

    def triangulate(self, cams, pts):
        """triangulation3D: cams (B, M, 3, 4) or (M, 3, 4) shared; pts (B, N, 2M).  -> (B, 4, N) unit homogeneous."""
        self._begin()
        pts = self._t(pts); B, N, M2 = pts.shape; M = M2 // 2
        cams = self._cams_cm(self._t(cams))
        stride = 12 * M if cams.dim() == 4 else 0
        X = torch.empty((B, N, 4), dtype=torch.float64, device=pts.device)
        _check(self.lib, self.lib.tff_triangulate_batch_dev(self.handle, self._p(cams), stride, self._p(pts), B, M, N, self._p(X)),
               "tff_triangulate_batch_dev")
        return X.transpose(1, 2)

    def repr_error(self, cams, corresp, pts3d=None):
        """ReprError: cams (B, 3, 3, 4) or (3, 3, 4); corresp (B, N, 6) or (N, 6) shared; pts3d (B, 3, N) or None."""
        self._begin()
        cams = self._cams_cm(self._t(cams))
        cstride = 36 if cams.dim() == 4 else 0
        corresp = self._t(corresp)
        N = corresp.shape[-2]
        B = cams.shape[0] if cstride else (corresp.shape[0] if corresp.dim() == 3 else 1)
        pstride = 6 * N if corresp.dim() == 3 else 0
        p3 = self._t(pts3d).transpose(1, 2).contiguous() if pts3d is not None else None
        err = torch.empty(B, dtype=torch.float64, device=corresp.device)
        _check(self.lib, self.lib.tff_repr_error_batch_dev(self.handle, self._p(cams), cstride, self._p(corresp), pstride,
                                                           self._p(p3), B, N, self._p(err)), "tff_repr_error_batch_dev")
        return err

    def inlier_count(self, scene, calm, R_t_2, R_t_3, threshold=1.0, with_error=False):
        """Inlier counts (experiments_real.m:94-98 rule) of B pose hypotheses against one scene (Ns, 6); their MSAC scores after set_score("msac")."""
        self._begin()
        scene = self._t(scene); Ns = scene.shape[0]
        calm = self._t(calm).t().contiguous().reshape(27)
        r2 = self._cams_cm(self._t(R_t_2)); r3 = self._cams_cm(self._t(R_t_3)); B = r2.shape[0]
        cnt = torch.empty(B, dtype=torch.int32, device=scene.device)
        err = torch.empty(B, dtype=torch.float64, device=scene.device) if with_error else None
        _check(self.lib, self.lib.tff_inlier_count_batch_dev(self.handle, self._p(scene), Ns, self._p(calm), self._p(r2), self._p(r3), B,
                                                             float(threshold), self._p(cnt), self._p(err)), "tff_inlier_count_batch_dev")
        return (cnt, err) if with_error else cnt

    def transform_tft(self, T, M1, M2, M3, inverse=0):
        """transform_TFT: T (B,3,3,3) indexed [b,j,k,i]; M1..M3 (3,3) shared or (B,3,3)."""
        self._begin()
        T = self._t(T); B = T.shape[0]
        Tv = T.permute(0, 3, 2, 1).contiguous()                               # -> flat index j + 3k + 9i
        Ms = [self._t(M).transpose(-1, -2).contiguous() for M in (M1, M2, M3)]
        stride = 9 if Ms[0].dim() == 3 else 0
        out = torch.empty((B, 27), dtype=torch.float64, device=T.device)
        _check(self.lib, self.lib.tff_transform_tft_batch_dev(self.handle, self._p(Tv), self._p(Ms[0]), self._p(Ms[1]), self._p(Ms[2]),
                                                              stride, B, int(inverse), self._p(out)), "tff_transform_tft_batch_dev")
        return out.reshape(B, 3, 3, 3).permute(0, 3, 2, 1)

    def rt_from_tft(self, T, calm, corresp):
        """R_t_from_TFT: T (B,3,3,3) [b,j,k,i] in pixel coordinates, calm (9,3), corresp (B,N,6)."""
        self._begin()
        T = self._t(T); B = T.shape[0]
        Tv = T.permute(0, 3, 2, 1).contiguous()
        corresp = self._t(corresp); N = corresp.shape[1]
        calm = self._t(calm).t().contiguous().reshape(27)
        Rt2 = torch.empty((B, 12), dtype=torch.float64, device=T.device); Rt3 = torch.empty_like(Rt2)
        st = torch.zeros(B, dtype=torch.int32, device=T.device)
        _check(self.lib, self.lib.tff_rt_from_tft_batch_dev(self.handle, self._p(Tv), self._p(calm), 0, self._p(corresp), B, N,
                                                            self._p(Rt2), self._p(Rt3), self._p(st)), "tff_rt_from_tft_batch_dev")
        return Rt2.reshape(B, 4, 3).transpose(1, 2), Rt3.reshape(B, 4, 3).transpose(1, 2), st

    def linear_tft(self, corresp):
        """linearTFT on the given (already normalised, if desired) points: corresp (B,N,6) -> T (B,3,3,3), P2, P3 (B,3,4)."""
        self._begin()
        corresp = self._t(corresp); B, N, _ = corresp.shape
        T = torch.empty((B, 27), dtype=torch.float64, device=corresp.device)
        P2 = torch.empty((B, 12), dtype=torch.float64, device=corresp.device); P3 = torch.empty_like(P2)
        st = torch.zeros(B, dtype=torch.int32, device=corresp.device)
        _check(self.lib, self.lib.tff_linear_tft_batch_dev(self.handle, self._p(corresp), B, N, self._p(T), self._p(P2), self._p(P3),
                                                           self._p(st)), "tff_linear_tft_batch_dev")
        return T.reshape(B, 3, 3, 3).permute(0, 3, 2, 1), P2.reshape(B, 4, 3).transpose(1, 2), P3.reshape(B, 4, 3).transpose(1, 2), st

    def linear_f(self, corresp, refine=False):
        """linearF (refine=False) / optimF (refine=True) for view pairs (1,2), (1,3): corresp (B,N,6) -> F21, F31 (B,3,3), iter, status."""
        self._begin()
        corresp = self._t(corresp); B, N, _ = corresp.shape
        F21 = torch.empty((B, 9), dtype=torch.float64, device=corresp.device); F31 = torch.empty_like(F21)
        it = torch.zeros(B, dtype=torch.int32, device=corresp.device); st = torch.zeros_like(it)
        _check(self.lib, self.lib.tff_linear_f_batch_dev(self.handle, self._p(corresp), B, N, int(bool(refine)), self._p(F21), self._p(F31),
                                                         self._p(it), self._p(st)), "tff_linear_f_batch_dev")
        return F21.reshape(B, 3, 3).transpose(1, 2), F31.reshape(B, 3, 3).transpose(1, 2), it, st

    def bundle_adjust(self, calm, R_t_2, R_t_3, corresp, reconst0=None, loss=None, scale=None, cov=False, point_cov=False):
        """BundleAdjustment for B triplets: calm (9,3) or (B,9,3); R_t_2, R_t_3 (B,3,4); corresp (B,N,6); reconst0 (B,3,N) or None.
        -> dict(R_t_2, R_t_3 (B,3,4), Reconst (B,3,N), iter, repr_err, status).
        loss = "huber" or "cauchy" with scale = c in pixels (tff_bundle_adjust_loss_batch_dev, include/tftfund_loss.h): the adjustment minimises
        sum rho(|pixel residual|^2) by reweighted Levenberg-Marquardt, repr_err is the square root of that sum, and weight (B,N), rho' at the final
        parameters, joins the dict.  Without a loss nothing changes.
        cov=True (tff_bundle_adjust_cov_batch_dev, include/tftfund_cov.h): cov (B,12,12), the covariance of (angles2, angles3, t2, t3) in the gauge
        |t2| = 1, and sigma0 (B,) join the dict; point_cov=True adds them and point_cov (B,N,6), every point's 3x3 block packed xx xy xz yy yz zz.
        They are what ba_covariance gives on this call's outputs, and every other output keeps its bits."""
        robust = _check_loss(loss, scale)
        self._begin()
        corresp = self._t(corresp); B, N, _ = corresp.shape
        dev = corresp.device
        calm = self._t(calm)
        if calm.dim() == 2:
            calm_cm, stride = calm.t().contiguous().reshape(27), 0
        else:
            calm_cm, stride = calm.transpose(1, 2).contiguous().reshape(B * 27), 27
        r2 = self._cams_cm(self._t(R_t_2)); r3 = self._cams_cm(self._t(R_t_3))
        x0 = self._t(reconst0).transpose(1, 2).contiguous() if reconst0 is not None else None
        o2 = torch.empty((B, 12), dtype=torch.float64, device=dev); o3 = torch.empty_like(o2)
        rec = torch.empty((B, N, 3), dtype=torch.float64, device=dev)
        it = torch.zeros(B, dtype=torch.int32, device=dev); st = torch.zeros_like(it)
        err = torch.empty(B, dtype=torch.float64, device=dev)
        a = (self.handle, self._p(calm_cm), stride, self._p(r2), self._p(r3), self._p(corresp), B, N, self._p(x0), self._p(o2), self._p(o3), self._p(rec),
             self._p(it), self._p(err), self._p(st))
        out = dict(R_t_2=o2.reshape(B, 4, 3).transpose(1, 2), R_t_3=o3.reshape(B, 4, 3).transpose(1, 2), Reconst=rec.transpose(1, 2),
                   iter=it, repr_err=err, status=st)
        if robust is not None:
            out["weight"] = torch.empty((B, N), dtype=torch.float64, device=dev)
        if cov or point_cov:
            out["cov"] = torch.empty((B, 12, 12), dtype=torch.float64, device=dev); out["sigma0"] = torch.empty(B, dtype=torch.float64, device=dev)
            if point_cov:
                out["point_cov"] = torch.empty((B, N, 6), dtype=torch.float64, device=dev)
            _check(self.lib, self.lib.tff_bundle_adjust_cov_batch_dev(*a, *(robust or (0, 0.0)), self._p(out.get("weight")), self._p(out["cov"]), self._p(out["sigma0"]),
                                                                      self._p(out.get("point_cov"))), "tff_bundle_adjust_cov_batch_dev")
        elif robust is None:
            _check(self.lib, self.lib.tff_bundle_adjust_batch_dev(*a), "tff_bundle_adjust_batch_dev")
        else:
            _check(self.lib, self.lib.tff_bundle_adjust_loss_batch_dev(*a, robust[0], robust[1], self._p(out["weight"])), "tff_bundle_adjust_loss_batch_dev")
        return out

    def ba_covariance(self, calm, R_t_2, R_t_3, corresp, reconst, loss=None, scale=None, point_cov=False):
        """The covariance of a three-view bundle adjustment AT the given poses and points (tff_ba_covariance_batch_dev, include/tftfund_cov.h; no
        iteration is run): calm (9,3) or (B,9,3); R_t_2, R_t_3 (B,3,4); corresp (B,N,6); reconst (B,3,N), as bundle_adjust takes and returns them;
        loss, scale as there.  -> dict(cov (B,12,12), sigma0 (B,)[, point_cov (B,N,6)]): cov is that of (angles2, angles3, t2, t3) -- the angles of
        R = Rx Ry Rz, see euler_cov_to_rotvec -- in the gauge |t2| = 1, sigma0^2 = r'r / (3N - 11) (normalised units without a loss, pixels with
        one); NaN for N <= 3 and for non-finite poses."""
        robust = _check_loss(loss, scale) or (0, 0.0)
        self._begin()
        corresp = self._t(corresp); B, N, _ = corresp.shape
        dev = corresp.device
        calm = self._t(calm)
        if calm.dim() == 2:
            calm_cm, stride = calm.t().contiguous().reshape(27), 0
        else:
            calm_cm, stride = calm.transpose(1, 2).contiguous().reshape(B * 27), 27
        r2 = self._cams_cm(self._t(R_t_2)); r3 = self._cams_cm(self._t(R_t_3))
        x = self._t(reconst).transpose(1, 2).contiguous()
        if tuple(x.shape) != (B, N, 3):
            raise ValueError("reconst must be (B, 3, N)")
        out = dict(cov=torch.empty((B, 12, 12), dtype=torch.float64, device=dev), sigma0=torch.empty(B, dtype=torch.float64, device=dev))
        if point_cov:
            out["point_cov"] = torch.empty((B, N, 6), dtype=torch.float64, device=dev)
        _check(self.lib, self.lib.tff_ba_covariance_batch_dev(self.handle, self._p(calm_cm), stride, self._p(r2), self._p(r3), self._p(corresp), B, N, self._p(x),
                                                              robust[0], robust[1], self._p(out["cov"]), self._p(out["sigma0"]), self._p(out.get("point_cov"))),
               "tff_ba_covariance_batch_dev")
        return out

    def bundle_adjust_ragged(self, calm, R_t_2, R_t_3, corresp, offsets, mask=None, reconst0=None, reconst=True, loss=None, scale=None, cov=False,
                             point_cov=False, _cov_only=None):
        """BundleAdjustment for B items with different correspondence counts in one call (tff_bundle_adjust_ragged_*): corresp (Ntot, 6) packed,
        offsets (B + 1,) int64 with item b = corresp[offsets[b]:offsets[b + 1]] (see pack_ragged), mask None or (Ntot,) uint8 / bool (non-zero = use the
        correspondence: the `mask` of robust_pose_scenes), calm (9, 3) or (B, 9, 3), R_t_2, R_t_3 (B, 3, 4), reconst0 None or (Ntot, 3) (read where
        selected).  Item b gets bit for bit what bundle_adjust returns for its selected correspondences alone.  CUDA tensors in (offsets on the device)
        -> CUDA tensors out, no synchronisation; numpy in -> numpy out through the _host form (malformed offsets raise).
        Returns dict(R_t_2, R_t_3 (B,3,4), Reconst (Ntot,3) or None -- NaN where not selected --, iter, repr_err, used, status (B,)); per item
        ST_BAD_OFFSETS / ST_TOO_FEW (nothing selected) / ST_TOO_LARGE (more than BA_MAX_N selected) with NaN poses.
        loss, scale: as bundle_adjust (tff_bundle_adjust_loss_ragged_*); weight (Ntot,), packed like corresp, joins the dict: NaN where the mask
        deselects and over an item that failed.  Item b still equals bundle_adjust with the same loss on its selection, bit for bit.
        cov, point_cov: as bundle_adjust (tff_bundle_adjust_cov_ragged_*): cov (B,12,12), sigma0 (B,) and point_cov (Ntot,6), packed like corresp and NaN
        where not selected; NaN for an item that failed or has three or fewer selected.  They are ba_covariance_ragged on this call's outputs."""
        robust = _check_loss(loss, scale)
        want_cov = bool(cov or point_cov)
        host = isinstance(corresp, np.ndarray)
        if host:
            offsets = np.asarray(offsets)
            check_offsets(offsets)
            offsets = np.ascontiguousarray(offsets, dtype=np.int64)
            corresp = np.ascontiguousarray(corresp, dtype=np.float64)
            if corresp.ndim != 2 or corresp.shape[1] != 6:
                raise ValueError("corresp must be (Ntot, 6)")
            if offsets[-1] > corresp.shape[0]:
                raise ValueError("offsets[-1] = %d beyond the %d packed correspondences" % (offsets[-1], corresp.shape[0]))
        else:
            if not (isinstance(corresp, torch.Tensor) and corresp.is_cuda and corresp.dtype == torch.float64 and corresp.is_contiguous() and corresp.dim() == 2
                    and corresp.shape[1] == 6):
                raise ValueError("corresp must be a contiguous float64 CUDA tensor of shape (Ntot, 6)")
            if not (isinstance(offsets, torch.Tensor) and offsets.is_cuda and offsets.device == corresp.device and offsets.dtype == torch.int64
                    and offsets.dim() == 1 and offsets.shape[0] >= 1):
                raise ValueError("offsets must be a 1-D int64 tensor of B + 1 entries on the device of corresp")
            offsets = offsets.contiguous()
        B = offsets.shape[0] - 1
        ntot = corresp.shape[0]
        for name, a in (("R_t_2", R_t_2), ("R_t_3", R_t_3)):
            if tuple(a.shape) != (B, 3, 4):
                raise ValueError("%s must be (B, 3, 4) with B = %d" % (name, B))
        if mask is not None and tuple(mask.shape) != (ntot,):
            raise ValueError("mask must hold one flag per packed correspondence: (%d,)" % ntot)
        if reconst0 is not None and tuple(reconst0.shape) != (ntot, 3):
            raise ValueError("%s must be (Ntot, 3), packed like corresp" % ("reconst0" if _cov_only is None else "reconst"))
        if not isinstance(calm, (np.ndarray, torch.Tensor)) or tuple(calm.shape) not in ((9, 3), (B, 9, 3)):
            raise ValueError("CalM must be a (9, 3) or (B, 9, 3) array or tensor")
        if host:
            to_np = lambda a, dt=np.float64: np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=dt)
            calm_cm, stride = self._calm_cm_np(to_np(calm), B)
            r2 = np.ascontiguousarray(to_np(R_t_2).transpose(0, 2, 1)); r3 = np.ascontiguousarray(to_np(R_t_3).transpose(0, 2, 1))
            mk = None if mask is None else np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
            x0 = None if reconst0 is None else to_np(reconst0)
            o2 = np.empty((B, 12)); o3 = np.empty((B, 12))
            rec = np.full((ntot, 3), np.nan) if reconst else None
            it = np.zeros(B, dtype=np.int32); st = np.zeros(B, dtype=np.int32); used = np.zeros(B, dtype=np.int32); err = np.empty(B)
            ptr = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None
            a = (self.handle, ptr(corresp), ptr(offsets), ptr(mk), ptr(calm_cm), stride, ptr(r2), ptr(r3), ptr(x0), B, ptr(o2), ptr(o3), ptr(rec), ptr(it),
                 ptr(err), ptr(used), ptr(st))
            out = dict(R_t_2=o2.reshape(B, 4, 3).transpose(0, 2, 1), R_t_3=o3.reshape(B, 4, 3).transpose(0, 2, 1), Reconst=rec, iter=it, repr_err=err,
                       used=used, status=st)
            if _cov_only is not None:                                        # ba_covariance_ragged: the same arguments, no adjustment
                co = dict(cov=np.full((B, 12, 12), np.nan), sigma0=np.full(B, np.nan))
                if _cov_only:
                    co["point_cov"] = np.full((ntot, 6), np.nan)
                _check(self.lib, self.lib.tff_ba_covariance_ragged_host(self.handle, ptr(corresp), ptr(offsets), ptr(mk), ptr(calm_cm), stride, ptr(r2), ptr(r3), ptr(x0), B,
                                                                        *(robust or (0, 0.0)), ptr(co["cov"]), ptr(co["sigma0"]), ptr(co.get("point_cov"))),
                       "tff_ba_covariance_ragged_host")
                return co
            if robust is not None:
                out["weight"] = np.full(ntot, np.nan)
            if want_cov:
                out["cov"] = np.full((B, 12, 12), np.nan); out["sigma0"] = np.full(B, np.nan)
                if point_cov:
                    out["point_cov"] = np.full((ntot, 6), np.nan)
                _check(self.lib, self.lib.tff_bundle_adjust_cov_ragged_host(*a, *(robust or (0, 0.0)), ptr(out.get("weight")), ptr(out["cov"]), ptr(out["sigma0"]),
                                                                            ptr(out.get("point_cov"))), "tff_bundle_adjust_cov_ragged_host")
            elif robust is None:
                _check(self.lib, self.lib.tff_bundle_adjust_ragged_host(*a), "tff_bundle_adjust_ragged_host")
            else:
                _check(self.lib, self.lib.tff_bundle_adjust_loss_ragged_host(*a, robust[0], robust[1], ptr(out["weight"])), "tff_bundle_adjust_loss_ragged_host")
            return out
        dev = corresp.device
        calm_cm, stride = self._calm_scenes(calm, B, dev)
        on_dev = lambda a, dt: (torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a).to(device=dev, dtype=dt)
        r2 = on_dev(R_t_2, torch.float64).transpose(1, 2).contiguous(); r3 = on_dev(R_t_3, torch.float64).transpose(1, 2).contiguous()
        mk = None if mask is None else on_dev(mask, torch.uint8).contiguous()       # (bool -> 0 / 1)
        x0 = None if reconst0 is None else on_dev(reconst0, torch.float64).contiguous()
        o2 = torch.empty((B, 12), dtype=torch.float64, device=dev); o3 = torch.empty_like(o2)
        rec = torch.full((ntot, 3), float("nan"), dtype=torch.float64, device=dev) if reconst else None
        it = torch.zeros(B, dtype=torch.int32, device=dev); st = torch.zeros_like(it); used = torch.zeros_like(it)
        err = torch.empty(B, dtype=torch.float64, device=dev)
        self.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        a = (self.handle, self._p(corresp), self._p(offsets), ntot, self._p(mk), self._p(calm_cm), stride, self._p(r2), self._p(r3), self._p(x0), B,
             self._p(o2), self._p(o3), self._p(rec), self._p(it), self._p(err), self._p(used), self._p(st))
        out = dict(R_t_2=o2.reshape(B, 4, 3).transpose(1, 2), R_t_3=o3.reshape(B, 4, 3).transpose(1, 2), Reconst=rec, iter=it, repr_err=err, used=used,
                   status=st)
        nans = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)
        if _cov_only is not None:                                            # ba_covariance_ragged: the same arguments, no adjustment
            co = dict(cov=nans(B, 12, 12), sigma0=nans(B))
            if _cov_only:
                co["point_cov"] = nans(ntot, 6)
            _check(self.lib, self.lib.tff_ba_covariance_ragged_dev(self.handle, self._p(corresp), self._p(offsets), ntot, self._p(mk), self._p(calm_cm), stride, self._p(r2),
                                                                   self._p(r3), self._p(x0), B, *(robust or (0, 0.0)), self._p(co["cov"]), self._p(co["sigma0"]),
                                                                   self._p(co.get("point_cov"))), "tff_ba_covariance_ragged_dev")
            return co
        if robust is not None:
            out["weight"] = nans(ntot)
        if want_cov:
            out["cov"] = nans(B, 12, 12); out["sigma0"] = nans(B)
            if point_cov:
                out["point_cov"] = nans(ntot, 6)
            _check(self.lib, self.lib.tff_bundle_adjust_cov_ragged_dev(*a, *(robust or (0, 0.0)), self._p(out.get("weight")), self._p(out["cov"]), self._p(out["sigma0"]),
                                                                       self._p(out.get("point_cov"))), "tff_bundle_adjust_cov_ragged_dev")
        elif robust is None:
            _check(self.lib, self.lib.tff_bundle_adjust_ragged_dev(*a), "tff_bundle_adjust_ragged_dev")
        else:
            _check(self.lib, self.lib.tff_bundle_adjust_loss_ragged_dev(*a, robust[0], robust[1], self._p(out["weight"])), "tff_bundle_adjust_loss_ragged_dev")
        return out

    def ba_covariance_ragged(self, calm, R_t_2, R_t_3, corresp, offsets, reconst, mask=None, loss=None, scale=None, point_cov=False):
        """ba_covariance for B items with different correspondence counts in one call (tff_ba_covariance_ragged_*): the arguments of
        bundle_adjust_ragged, with reconst (Ntot, 3) the points, packed like corresp and read where selected -- what bundle_adjust_ragged returns as
        Reconst.  -> dict(cov (B,12,12), sigma0 (B,)[, point_cov (Ntot,6), NaN where not selected]).  Item b gets bit for bit what ba_covariance gives
        for its selected correspondences alone; an item with bad offsets, nothing or too little (three or fewer) selected, or NaN poses gets NaN.
        CUDA tensors in -> CUDA tensors out, no synchronisation; numpy in -> numpy out through the _host form."""
        if reconst is None:
            raise ValueError("the covariance is evaluated at given points: reconst must be (Ntot, 3)")
        return self.bundle_adjust_ragged(calm, R_t_2, R_t_3, corresp, offsets, mask=mask, reconst0=reconst, reconst=False, loss=loss, scale=scale,
                                         _cov_only=bool(point_cov))

    @staticmethod
    def _refined(out, r):
        """the refine step of robust_pose_scenes: the outputs of its one pose_batch_ragged call under their names"""
        out.update(R_t_2_refined=r["R_t_2"], R_t_3_refined=r["R_t_3"], T_refined=r["T"], iter_refined=r["iter"], status_refined=r["status"])

    @staticmethod
    def _check_polish(polish_loss, polish_scale, polish_all, threshold, polish=True, polish_cov=False):
        """the polish arguments of the robust calls -> (loss, scale, all matches, with the covariance)"""
        robust = _check_loss(polish_loss, polish_scale, "polish_loss", threshold)
        if polish_all and robust is None:
            raise ValueError("polish_all=True adjusts over all matches of a scene, wrong ones included: it needs a polish_loss")
        if polish_cov and not polish:
            raise ValueError("polish_cov=True is the covariance of the polished pose: it needs polish=True")
        return (polish_loss, None if robust is None else robust[1], bool(polish_all), bool(polish_cov))

    def _polish(self, out, calm, scenes, offsets, single, how=(None, None, False, False)):
        """the polish of robust_pose / robust_pose_scenes: ONE bundle_adjust_ragged call on the result's poses and mask (how: _check_polish -- with a
        loss, and then over the mask or over all matches)"""
        r2, r3 = out["R_t_2"], out["R_t_3"]
        if single:
            r2, r3 = r2[None], r3[None]
        ba = self.bundle_adjust_ragged(calm, r2, r3, scenes, offsets, mask=None if how[2] else out["mask"], reconst=False, loss=how[0], scale=how[1], cov=how[3])
        pick = (lambda a: a[0]) if single else (lambda a: a)
        out.update(R_t_2_polished=pick(ba["R_t_2"]), R_t_3_polished=pick(ba["R_t_3"]), iter_polished=pick(ba["iter"]),
                   repr_err_polished=pick(ba["repr_err"]), status_polished=pick(ba["status"]))
        if how[0] is not None:
            out["weight_polished"] = ba["weight"]                            # packed like mask
        if how[3]:
            out.update(cov_polished=pick(ba["cov"]), sigma0_polished=pick(ba["sigma0"]))
        return out

    def bundle_adjust_views(self, calm, R_t_0, corresp, reconst0=None, missing="view", loss=None, scale=None, cov=False, point_cov=False):
        """BundleAdjustment for B problems of M = 2 .. 6 views: calm (3M,3) or (B,3M,3); R_t_0 (B,3M,4), first camera included and free; corresp
        (B,N,2M), NaN = not seen; reconst0 (B,3,N) or None.  -> dict(R_t (B,3M,4), Reconst (B,3,N), iter, repr_err, status).
        missing="view" (tff_bundle_adjust_views_batch_dev): a NaN drops the whole view, as the reference's code does.
        missing="point" (tff_bundle_adjust_tracks_batch_dev, include/tftfund_tracks.h): a non-finite observation means that this point is not seen in
        this view, as the reference's header documents; a point with fewer than two observations is dropped (its Reconst column is NaN), and `used`
        (B,) int32, the number of points taking part, joins the dict.  An all-NaN column is inert: pad problems of different N with such columns.
        loss="huber" | "cauchy" with scale (pixels), missing="point" only (tff_bundle_adjust_tracks_loss_batch_dev, include/tftfund_tracks_loss.h): the
        loss is taken per OBSERVATION, repr_err is sqrt(sum rho) in pixels, and `weight` (B,N,M) joins the dict: rho' of every observation at the final
        parameters, NaN where there is no observation, over a dropped point and over an item whose status is not 0.
        cov=True, missing="point" only (tff_bundle_adjust_tracks_cov_batch_dev, include/tftfund_tracks_cov.h): cov (B,P,P), P = 6 (M - 1), the covariance
        of (angles of cameras 2..M, their translations) in the gauge |t2| = 1, and sigma0 (B,) join the dict; point_cov=True adds them and point_cov
        (B,N,6), every point's 3x3 block packed xx xy xz yy yz zz, NaN over a dropped point.  They are what ba_tracks_covariance gives on this call's
        outputs, and every other output keeps its bits."""
        if missing not in ("view", "point"):
            raise ValueError('missing must be "view" or "point"')
        _check_tracks_loss(missing, loss, scale)                             # (before a device is touched)
        if (cov or point_cov) and missing != "point":
            raise ValueError('a covariance needs missing="point": the whole-view call has none')
        if missing == "point":                                               # (the shapes, before a device is touched)
            cs = tuple(corresp.shape)
            if len(cs) != 3 or cs[2] % 2 or not 2 <= cs[2] // 2 <= 6:
                raise ValueError("corresp must be (B,N,2M) with M = 2 .. 6 views")
            if tuple(R_t_0.shape) != (cs[0], 3 * cs[2] // 2, 4) or tuple(calm.shape) not in ((3 * cs[2] // 2, 3), (cs[0], 3 * cs[2] // 2, 3)):
                raise ValueError("M views: corresp (B,N,2M), R_t_0 (B,3M,4), calm (3M,3) or (B,3M,3)")
            if reconst0 is not None and tuple(reconst0.shape) != (cs[0], 3, cs[1]):
                raise ValueError("reconst0 must be (B,3,N)")
        self._begin()
        corresp = self._t(corresp); B, N, M2 = corresp.shape
        M = M2 // 2
        dev = corresp.device
        calm = self._t(calm)
        if calm.dim() == 2:
            calm_cm, stride = calm.t().contiguous().reshape(9 * M), 0
        else:
            calm_cm, stride = calm.transpose(1, 2).contiguous().reshape(B * 9 * M), 9 * M
        rt = self._t(R_t_0)
        if M2 != 2 * M or tuple(rt.shape) != (B, 3 * M, 4) or calm_cm.numel() != (9 * M if stride == 0 else B * 9 * M):
            raise ValueError("M views: corresp (B,N,2M), R_t_0 (B,3M,4), calm (3M,3) or (B,3M,3)")
        rt_cm = rt.transpose(1, 2).contiguous()
        x0 = self._t(reconst0).transpose(1, 2).contiguous() if reconst0 is not None else None
        out = torch.empty((B, 4, 3 * M), dtype=torch.float64, device=dev)
        rec = torch.empty((B, N, 3), dtype=torch.float64, device=dev)
        it = torch.zeros(B, dtype=torch.int32, device=dev); st = torch.zeros_like(it)
        err = torch.empty(B, dtype=torch.float64, device=dev)
        if cov or point_cov:
            used = torch.zeros_like(it)
            res = dict(R_t=out.transpose(1, 2), Reconst=rec.transpose(1, 2), iter=it, repr_err=err, used=used, status=st)
            if loss is not None:
                res["weight"] = torch.empty((B, N, M), dtype=torch.float64, device=dev)
            P = 6 * (M - 1)
            res["cov"] = torch.empty((B, P, P), dtype=torch.float64, device=dev); res["sigma0"] = torch.empty(B, dtype=torch.float64, device=dev)
            if point_cov:
                res["point_cov"] = torch.empty((B, N, 6), dtype=torch.float64, device=dev)
            _check(self.lib, self.lib.tff_bundle_adjust_tracks_cov_batch_dev(self.handle, M, self._p(calm_cm), stride, self._p(rt_cm), self._p(corresp), B, N,
                                                                             self._p(x0), self._p(out), self._p(rec), self._p(it), self._p(err), self._p(used),
                                                                             self._p(st), LOSS_IDS[loss] if loss is not None else 0,
                                                                             float(scale) if loss is not None else 0.0, self._p(res.get("weight")),
                                                                             self._p(res["cov"]), self._p(res["sigma0"]), self._p(res.get("point_cov"))),
                   "tff_bundle_adjust_tracks_cov_batch_dev")
            return res
        if missing == "point" and loss is not None:
            used = torch.zeros_like(it)
            weight = torch.empty((B, N, M), dtype=torch.float64, device=dev)
            _check(self.lib, self.lib.tff_bundle_adjust_tracks_loss_batch_dev(self.handle, M, self._p(calm_cm), stride, self._p(rt_cm), self._p(corresp), B, N,
                                                                              self._p(x0), self._p(out), self._p(rec), self._p(it), self._p(err), self._p(used),
                                                                              self._p(st), LOSS_IDS[loss], float(scale), self._p(weight)),
                   "tff_bundle_adjust_tracks_loss_batch_dev")
            return dict(R_t=out.transpose(1, 2), Reconst=rec.transpose(1, 2), iter=it, repr_err=err, used=used, status=st, weight=weight)
        if missing == "point":
            used = torch.zeros_like(it)
            _check(self.lib, self.lib.tff_bundle_adjust_tracks_batch_dev(self.handle, M, self._p(calm_cm), stride, self._p(rt_cm), self._p(corresp), B, N,
                                                                         self._p(x0), self._p(out), self._p(rec), self._p(it), self._p(err), self._p(used),
                                                                         self._p(st)),
                   "tff_bundle_adjust_tracks_batch_dev")
            return dict(R_t=out.transpose(1, 2), Reconst=rec.transpose(1, 2), iter=it, repr_err=err, used=used, status=st)
        _check(self.lib, self.lib.tff_bundle_adjust_views_batch_dev(self.handle, M, self._p(calm_cm), stride, self._p(rt_cm), self._p(corresp), B, N,
                                                                    self._p(x0), self._p(out), self._p(rec), self._p(it), self._p(err), self._p(st)),
               "tff_bundle_adjust_views_batch_dev")
        return dict(R_t=out.transpose(1, 2), Reconst=rec.transpose(1, 2), iter=it, repr_err=err, status=st)

    def ba_tracks_covariance(self, calm, R_t, corresp, reconst, loss=None, scale=None, point_cov=False):
        """The covariance of a bundle adjustment over tracks AT the given poses and points (tff_ba_tracks_covariance_batch_dev,
        include/tftfund_tracks_cov.h; no iteration is run): calm (3M,3) or (B,3M,3); R_t (B,3M,4), first camera free, any common scale; corresp
        (B,N,2M), non-finite = not seen; reconst (B,3,N) in the frame of R_t, as bundle_adjust_views(..., missing="point") takes and returns them; loss,
        scale as there.  -> dict(cov (B,P,P), sigma0 (B,)[, point_cov (B,N,6)]), P = 6 (M - 1): cov is that of (angles of cameras 2..M, their
        translations) -- the angles of R = Rx Ry Rz, see euler_cov_to_rotvec_views -- in the output frame, camera 1 = [I|0] and |t2| = 1; the rows and
        columns of a camera nobody sees are 0; sigma0^2 = r'r / dof (normalised units without a loss, pixels with one).  NaN where there is no
        redundancy, for non-finite poses or points, and where view 2 is not seen."""
        _check_tracks_loss("point", loss, scale)                             # (before a device is touched)
        cs = tuple(corresp.shape)
        if len(cs) != 3 or cs[2] % 2 or not 2 <= cs[2] // 2 <= 6:
            raise ValueError("corresp must be (B,N,2M) with M = 2 .. 6 views")
        if tuple(R_t.shape) != (cs[0], 3 * cs[2] // 2, 4) or tuple(calm.shape) not in ((3 * cs[2] // 2, 3), (cs[0], 3 * cs[2] // 2, 3)):
            raise ValueError("M views: corresp (B,N,2M), R_t (B,3M,4), calm (3M,3) or (B,3M,3)")
        if reconst is None or tuple(reconst.shape) != (cs[0], 3, cs[1]):
            raise ValueError("reconst must be (B,3,N)")
        self._begin()
        corresp = self._t(corresp); B, N, M2 = corresp.shape
        M = M2 // 2
        dev = corresp.device
        calm = self._t(calm)
        if calm.dim() == 2:
            calm_cm, stride = calm.t().contiguous().reshape(9 * M), 0
        else:
            calm_cm, stride = calm.transpose(1, 2).contiguous().reshape(B * 9 * M), 9 * M
        rt_cm = self._t(R_t).transpose(1, 2).contiguous()
        x = self._t(reconst).transpose(1, 2).contiguous()
        P = 6 * (M - 1)
        out = dict(cov=torch.empty((B, P, P), dtype=torch.float64, device=dev), sigma0=torch.empty(B, dtype=torch.float64, device=dev))
        if point_cov:
            out["point_cov"] = torch.empty((B, N, 6), dtype=torch.float64, device=dev)
        _check(self.lib, self.lib.tff_ba_tracks_covariance_batch_dev(self.handle, M, self._p(calm_cm), stride, self._p(rt_cm), self._p(corresp), B, N, self._p(x),
                                                                     LOSS_IDS[loss] if loss is not None else 0, float(scale) if loss is not None else 0.0,
                                                                     self._p(out["cov"]), self._p(out["sigma0"]), self._p(out.get("point_cov"))),
               "tff_ba_tracks_covariance_batch_dev")
        return out

    def pose_sampled(self, method, scene, calm, sample_idx):
        """Minimal-sample hypotheses (config 4): scene (Ns, 6), sample_idx (B, n) int32 -> R_t_2, R_t_3 (B,3,4), T, status."""
        self._begin()
        scene = self._t(scene); Ns = scene.shape[0]
        idx = self._t(sample_idx, torch.int32); B, n = idx.shape
        calm = self._t(calm).t().contiguous().reshape(27)
        Rt2 = torch.empty((B, 12), dtype=torch.float64, device=scene.device); Rt3 = torch.empty_like(Rt2)
        T = torch.empty((B, 27), dtype=torch.float64, device=scene.device)
        st = torch.zeros(B, dtype=torch.int32, device=scene.device)
        fn = {"LinearTFTPoseEstimation": self.lib.tff_linear_tft_pose_sampled_dev,
              "LinearFPoseEstimation": self.lib.tff_linear_f_pose_sampled_dev}[method]
        _check(self.lib, fn(self.handle, self._p(scene), Ns, self._p(calm), self._p(idx), B, n, self._p(Rt2), self._p(Rt3), self._p(T),
                            self._p(st)), "pose_sampled")
        return dict(R_t_2=Rt2.reshape(B, 4, 3).transpose(1, 2), R_t_3=Rt3.reshape(B, 4, 3).transpose(1, 2),
                    T=T.reshape(B, 3, 3, 3).permute(0, 3, 2, 1), status=st, _raw=(Rt2, Rt3, T))

    # ---- matches with outliers ------------------------------------------------------------------------
    def sample_indices(self, seed, first, B, n, Ns):
        """tff_sample_indices_dev: (B, n) int32 CUDA tensor, row b = the n distinct indices of hypothesis first + b (see sample_indices_reference)."""
        self._begin()
        out = torch.empty((max(int(B), 0), max(int(n), 0)), dtype=torch.int32, device=torch.device("cuda", self.device))
        _check(self.lib, self.lib.tff_sample_indices_dev(self.handle, int(seed), int(first), int(B), int(n), int(Ns), self._p(out)),
               "tff_sample_indices_dev")
        return out

    def sample_indices_guided(self, seed, first, B, n, order, growth):
        """tff_sample_indices_guided_dev: (B, n) int32 CUDA tensor, row b = the indices of hypothesis first + b under the guided (PROSAC) sampler for the
        scene whose ranking, best first, is order (Ns,) int32 (see sample_indices_guided_reference)."""
        g = _check_growth(growth)
        self._begin()
        order = self._t(order, torch.int32)
        if order.dim() != 1:
            raise ValueError("order must be (Ns,)")
        out = torch.empty((max(int(B), 0), max(int(n), 0)), dtype=torch.int32, device=torch.device("cuda", self.device))
        _check(self.lib, self.lib.tff_sample_indices_guided_dev(self.handle, int(seed), int(first), int(B), int(n), order.shape[0], self._p(order), g,
                                                                self._p(out)), "tff_sample_indices_guided_dev")
        return out

    @staticmethod
    def _check_guided(scenes, order, quality, growth):
        """order= / quality= / growth= of robust_pose and robust_pose_scenes, judged before the library or a device is touched: None without a ranking,
        else (the name given, the array, growth)"""
        if order is None and quality is None:
            return None
        if order is not None and quality is not None:
            raise ValueError("pass at most one of order and quality")
        g = _check_growth(growth)
        what, a = ("order", order) if order is not None else ("quality", quality)
        if isinstance(scenes, np.ndarray):
            if not isinstance(a, np.ndarray):
                raise ValueError("%s must be a numpy array when the scenes are one (the host path)" % what)
            integer, floating = np.issubdtype(a.dtype, np.integer) and a.dtype == np.int32, np.issubdtype(a.dtype, np.floating)
        else:
            if not (isinstance(a, torch.Tensor) and isinstance(scenes, torch.Tensor) and a.is_cuda and a.device == scenes.device):
                raise ValueError("%s must be a CUDA tensor on the device of the scenes (the device path)" % what)
            integer, floating = a.dtype == torch.int32, a.is_floating_point()
        if a.ndim != 1 or a.shape[0] != scenes.shape[0]:
            raise ValueError("%s must be (Ntot,): one entry per packed correspondence" % what)
        if what == "order" and not integer:
            raise ValueError("order must be int32")
        if what == "quality" and not floating:
            raise ValueError("quality must be a float array")
        return what, a, g

    def inlier_mask(self, scene, calm, R_t_2, R_t_3, threshold, with_counts=False):
        """Inlier flags (B, Ns) uint8 of B pose hypotheses against one scene (Ns, 6), by the rule of inlier_count: the row sums are its counts."""
        self._begin()
        scene = self._t(scene); Ns = scene.shape[0]
        calm = self._t(calm).t().contiguous().reshape(27)
        r2 = self._cams_cm(self._t(R_t_2)); r3 = self._cams_cm(self._t(R_t_3)); B = r2.shape[0]
        mask = torch.empty((B, Ns), dtype=torch.uint8, device=scene.device)
        cnt = torch.empty(B, dtype=torch.int32, device=scene.device) if with_counts else None
        _check(self.lib, self.lib.tff_inlier_mask_batch_dev(self.handle, self._p(scene), Ns, self._p(calm), self._p(r2), self._p(r3), B,
                                                            float(threshold), self._p(mask), self._p(cnt)), "tff_inlier_mask_batch_dev")
        return (mask, cnt) if with_counts else mask

    def robust_pose(self, method, scene, calm, n_hyp, threshold, seed=0, n_sample=None, candidates=16, lo_rounds=2, refine=None, polish=False,
                    confidence=None, first_round=256, order=None, quality=None, growth=200000, polish_loss=None, polish_scale=None, polish_all=False,
                    polish_cov=False):
        """Pose from matches with outliers (tff_robust_pose_*): n_hyp minimal-sample hypotheses of `method` (LinearTFT / LinearF), the `candidates`
        best refitted on their inliers `lo_rounds` times, the best one returned.  scene (Ns, 6), calm (9, 3), threshold in pixels per coordinate.
        Returns dict(R_t_2 (3,4), R_t_3 (3,4), T (3,3,3) [j,k,i], mask (Ns,) uint8, inliers, hypothesis, refits, candidates, status): CUDA tensors in
        -> CUDA tensors (0-d for the five scalars) and no synchronisation; numpy in -> numpy / ints (the _host form).  refine = a name in POSE_METHODS:
        that method once on the final inliers through pose_batch (reads the count on the host), as R_t_2_refined, R_t_3_refined, T_refined,
        iter_refined, status_refined.  polish=True: BundleAdjustment on the pose and its inliers in one more call (bundle_adjust_ragged with the mask and the
        offsets [0, Ns], built on the device; no synchronisation and no copy on the device path), as R_t_2_polished, R_t_3_polished, iter_polished, repr_err_polished, status_polished.
        After set_score("msac") the hypotheses are ranked, refits adopted and the winner picked by the MSAC score, and `score` joins the dict: that of the
        returned pose, from one more inlier_count call (0-d CUDA tensor, no synchronisation / int; -1 without a pose).  mask and inliers stay the hard rule.
        confidence = c in (0, 1): the early stop of robust_pose_scenes for this one scene (the S = 1 call with the offsets [0, Ns]): n_hyp is the cap,
        first_round the first round's length, and n_hyp_used joins the dict; the result is that of this call with n_hyp = n_hyp_used.
        order= (Ns,) int32, the matches best first, or quality= (Ns,) float, higher is better, with growth: the guided sampler of robust_pose_scenes for
        this one scene (the S = 1 call with the offsets [0, Ns]); n_hyp_used joins the dict only with a confidence.  Without them nothing changes.
        polish_loss, polish_scale, polish_all: as robust_pose_scenes; weight_polished (Ns,) joins the dict.  polish_cov=True: cov_polished (12,12) and
        sigma0_polished, as robust_pose_scenes."""
        how = self._check_polish(polish_loss, polish_scale, polish_all, threshold, polish, polish_cov)
        if method not in ROBUST_METHODS:
            raise ValueError("robust_pose draws its hypotheses with LinearTFTPoseEstimation or LinearFPoseEstimation, not %r" % (method,))
        if refine is not None and refine not in POSE_METHODS:
            raise ValueError("unknown refine method %r" % (refine,))
        adaptive = None if confidence is None else _check_adaptive(confidence, first_round)
        guided = self._check_guided(scene, order, quality, growth)
        host = isinstance(scene, np.ndarray)
        if host:
            sc = np.ascontiguousarray(scene, dtype=np.float64)
            if sc.ndim != 2 or sc.shape[1] != 6:
                raise ValueError("scene must be (Ns, 6)")
            if not isinstance(calm, torch.Tensor):
                calm = np.asarray(calm, dtype=np.float64)
            if tuple(calm.shape) == (1, 9, 3):                               # (the numpy form has always taken the batch-of-one CalM of pose_batch)
                calm = calm[0]
        else:
            if not (scene.is_cuda and scene.dtype == torch.float64 and scene.is_contiguous() and scene.dim() == 2 and scene.shape[1] == 6):
                raise ValueError("scene must be a contiguous float64 CUDA tensor of shape (Ns, 6)")
            sc = scene
            if isinstance(calm, np.ndarray):
                calm = torch.from_numpy(np.ascontiguousarray(calm, dtype=np.float64))
        if tuple(calm.shape) != (9, 3):
            raise ValueError("CalM must be (9, 3)")
        Ns = sc.shape[0]
        offsets = None
        if not host:
            dev = sc.device
            calm = calm.to(device=dev, dtype=torch.float64)
            if polish or adaptive or guided:
                offsets = torch.arange(2, dtype=torch.int64, device=dev) * Ns   # [0, Ns], made on the device
        elif polish or adaptive or guided:
            offsets = np.array([0, Ns], dtype=np.int64)
        if adaptive or guided:                                               # the S = 1 scenes call ...
            more = dict(confidence=adaptive[0], first_round=adaptive[1]) if adaptive else {}
            r = self.robust_pose_scenes(method, sc, offsets, calm, n_hyp, threshold, seed=seed, n_sample=n_sample, candidates=candidates,
                                        lo_rounds=lo_rounds, ns_max=Ns, order=order, quality=quality, growth=growth, **more)
        else:                                                                # ... or the one-scene entry point, its outputs those of S = 1
            args = (int(seed), int(n_hyp), 0 if n_sample is None else int(n_sample), float(threshold), int(candidates), int(lo_rounds))
            if host:
                calm_cm, p, name = self._calm_cm_np(calm, 1)[0], _np_ptr, "tff_robust_pose_host"
            else:
                calm_cm, p, name = calm.t().contiguous().reshape(27), self._p, "tff_robust_pose_dev"
                self.set_stream(torch.cuda.current_stream(dev).cuda_stream)
            o, r = self._robust_outputs(1, Ns, False, None if host else dev)
            _check(self.lib, getattr(self.lib, name)(self.handle, METHOD_IDS[method], p(sc), Ns, p(calm_cm), *args, *map(p, o[:5]), p(o[6])), name)
        # ... reshaped to the one-scene dict
        one = (lambda a: a[0].item()) if host else (lambda a: a[0])
        out = dict(R_t_2=r["R_t_2"][0], R_t_3=r["R_t_3"][0], T=r["T"][0], mask=r["mask"], inliers=one(r["inliers"]), hypothesis=one(r["hypothesis"]),
                   refits=one(r["refits"]), candidates=one(r["candidates"]), status=one(r["status"]))
        if "score" in r:
            out["score"] = one(r["score"])
        elif getattr(self, "_score", 0):                                     # the direct call: one more count call on the returned pose; no pose (NaN): -1
            count = lambda: self.inlier_count(sc, calm, out["R_t_2"][None], out["R_t_3"][None], threshold)[0]
            if host:
                out["score"] = int(count()) if out["status"] == 0 else -1
            else:
                sco = count()
                out["score"] = torch.where(out["status"] == 0, sco, torch.full_like(sco, -1))
        if adaptive:
            out["n_hyp_used"] = one(r["n_hyp_used"])
        # refine and polish, the same for both forms
        if refine is not None:                                               # (boolean indexing reads the count on the host)
            inl = sc[out["mask"] != 0] if host else sc[out["mask"] != 0].contiguous()
            r = self.pose_batch(refine, inl.reshape(1, -1, 6), calm, reconst=False)
            out.update(R_t_2_refined=r["R_t_2"][0], R_t_3_refined=r["R_t_3"][0], T_refined=r["T"][0], iter_refined=r["iter"][0],
                       status_refined=r["status"][0])
        if polish:
            self._polish(out, calm, sc, offsets, True, how)
            if host:
                out["iter_polished"] = int(out["iter_polished"]); out["status_polished"] = int(out["status_polished"])
                out["repr_err_polished"] = float(out["repr_err_polished"])
                if how[3]:
                    out["sigma0_polished"] = float(out["sigma0_polished"])
        return out

    @staticmethod
    def _robust_outputs(S, n_mask, with_used, dev):
        """the outputs of a robust call of S scenes -- numpy for the _host forms (dev None), else uninitialised tensors on dev, used alone zeroed (the
        library may leave it unwritten) -> (as the library takes them: Rt2 (S,12), Rt3, T (S,27), mask (n_mask,), info (S,4), used (S,) or None, status
        (S,); the dict of robust_pose_scenes over them: views that turn the column-major Rt and T into (S,3,4) and (S,3,3,3), numpy or torch alike)"""
        if dev is None:
            new = lambda dt, *shape: np.zeros(shape, dtype=dt)
        else:
            new = lambda dt, *shape: torch.empty(shape, dtype=getattr(torch, dt), device=dev)
        Rt2, Rt3, T, mask, info, st = new("float64", S, 12), new("float64", S, 12), new("float64", S, 27), new("uint8", n_mask), new("int32", S, 4), new("int32", S)
        out = dict(R_t_2=Rt2.reshape(S, 4, 3).swapaxes(1, 2), R_t_3=Rt3.reshape(S, 4, 3).swapaxes(1, 2), T=T.reshape(S, 3, 3, 3).swapaxes(1, 3), mask=mask,
                   inliers=info[:, 0], hypothesis=info[:, 1], refits=info[:, 2], candidates=info[:, 3], status=st)
        if with_used:
            out["n_hyp_used"] = new("int32", S) if dev is None else torch.zeros(S, dtype=torch.int32, device=dev)
        return (Rt2, Rt3, T, mask, info, out.get("n_hyp_used"), st), out

    def _calm_scenes(self, calm, S, dev):
        """(9, 3) or (S, 9, 3) numpy / torch CalM -> (column-major flat tensor on dev, calm_stride)"""
        if isinstance(calm, np.ndarray):
            calm = torch.from_numpy(np.ascontiguousarray(calm, dtype=np.float64))
        if not isinstance(calm, torch.Tensor) or tuple(calm.shape) not in ((9, 3), (S, 9, 3)):
            raise ValueError("CalM must be a (9, 3) or (S, 9, 3) array or tensor")
        if tuple(calm.shape) == (9, 3):
            calm_cm, stride = calm.t().contiguous().reshape(27), 0
        else:
            calm_cm, stride = calm.transpose(1, 2).contiguous().reshape(S * 27), 27
        return calm_cm.to(device=dev, dtype=torch.float64), stride

    def _robust_scenes_call(self, dev, mid, scenes, offsets, sizes, S, calm_cm, stride, scalars, adaptive, ranking):
        """the library call of robust_pose_scenes, _host (dev None) or _dev (sizes: the two it adds), assembled once: handle and inputs, the six scalars,
        confidence and first_round if any, ranking and growth if any, the outputs, used if the form has it, status -> the result dict"""
        p = _np_ptr if dev is None else self._p
        name = _ROBUST_SCENES_ENTRY[ranking is not None, adaptive is not None] + ("_host" if dev is None else "_dev")
        o, out = self._robust_outputs(S, scenes.shape[0], adaptive is not None, dev)
        a = (self.handle, mid, p(scenes), p(offsets)) + sizes + (S, p(calm_cm), stride) + scalars
        if ranking is not None:                                              # (rank, growth); without a confidence: 0.0, a fixed n_hyp
            a += (adaptive or (0.0, 0)) + (p(ranking[0]), ranking[1])
        elif adaptive is not None:
            a += adaptive
        a += tuple(map(p, o[:5]))
        if ranking is not None or adaptive is not None:
            a += (p(o[5]),)
        _check(self.lib, getattr(self.lib, name)(*a, p(o[6])), name)
        return out

    def robust_pose_scenes(self, method, scenes, offsets, calm, n_hyp, threshold, seed=0, n_sample=None, candidates=16, lo_rounds=2, ns_max=None,
                           polish=False, refine=None, confidence=None, first_round=256, order=None, quality=None, growth=200000, polish_loss=None,
                           polish_scale=None, polish_all=False, polish_cov=False):
        """robust_pose for S scenes in one call (tff_robust_pose_scenes_*): scenes (Ntot, 6) packed, offsets (S + 1,) int64 with scene s =
        scenes[offsets[s]:offsets[s + 1]] (see pack_ragged), calm (9, 3) shared or (S, 9, 3).  Scene s gets bit for bit what robust_pose returns for it alone
        with seed + s (wrapping uint64).  Returns dict(R_t_2, R_t_3 (S,3,4), T (S,3,3,3), mask (Ntot,) uint8 packed like the scenes, inliers, hypothesis,
        refits, candidates, status (S,)).  CUDA tensors in (offsets on the device) -> CUDA tensors out, no synchronisation when ns_max, a bound on every
        scene's size, is passed (it is computed from the offsets with one synchronisation otherwise); a scene with bad offsets or fewer correspondences than a
        sample gets ST_BAD_OFFSETS / ST_TOO_FEW.  numpy in -> numpy out through the _host form, which refuses malformed offsets.
        polish=True: BundleAdjustment on every scene's pose and inliers in ONE more call (bundle_adjust_ragged on the result's poses and mask), as
        R_t_2_polished, R_t_3_polished (S,3,4), iter_polished, repr_err_polished, status_polished (S,); a scene without a pose gets ST_TOO_FEW there.
        refine = a name in RAGGED_METHODS: that method on every scene's inliers in ONE pose_batch_ragged call (reconst=False), as R_t_2_refined, R_t_3_refined
        (S,3,4), T_refined (S,3,3,3), iter_refined, status_refined (S,): bit for bit what robust_pose(..., refine=...) gives for the scene alone; a scene
        without a pose has no inliers and gets ST_TOO_FEW and NaN.  On the device path the inliers are packed without reading a count (no
        synchronisation when ns_max is passed).  The polish keeps starting from the robust poses.
        After set_score("msac"): as robust_pose, with `score` (S,) from one more inlier_count_scenes call, -1 for a scene without a pose.
        confidence = c in (0, 1): the early stop (tff_robust_pose_scenes_adaptive_*).  Hypotheses are drawn in rounds ending at round_plan(c, n_hyp,
        first_round)[0] per scene, n_hyp being the cap, and a scene stops after the round at which adaptive_stop holds for its best hypothesis; n_hyp_used
        (S,) int32 joins the dict (0 for a scene that never ran), and scene s gets bit for bit what robust_pose gives for it alone with n_hyp =
        n_hyp_used[s] and seed + s.  Still no synchronisation on the device path.  Without a confidence nothing changes and the key is absent.
        order= or quality= (at most one): quality-guided (PROSAC) sampling, tff_robust_pose_scenes_guided_*.  order (Ntot,) int32 holds every scene's
        ranking, best first, as local indices 0 .. n_s - 1, packed like the scenes (numpy on the host path, a CUDA tensor on the device path); quality
        (Ntot,) float, higher is better and NaN last, is turned into it by stable sorts (order_from_quality; torch on the device path, no
        synchronisation).  The early hypotheses draw from the best-ranked matches, and after `growth` draws per scene the sampling is the uniform one
        (sample_indices_guided_reference is the definition).  Scene s still equals its own one-scene call with seed + s, and confidence, refine, polish
        and set_score("msac") compose as without a ranking; the stop rule is the existing one.  Without either argument growth is ignored.
        polish_loss = "huber" or "cauchy": the polish minimises that robust loss (bundle_adjust_ragged(..., loss=, scale=)) with polish_scale pixels,
        by default `threshold`; weight_polished (Ntot,), packed like mask, joins the dict.  polish_all=True passes no mask: the polish runs over all
        matches of every scene and the loss alone keeps the wrong ones down (refused without a loss).  A scene without a pose then enters the adjustment
        with its NaN poses and leaves it with ST_NONFINITE, NaN poses and NaN weights (under the mask: ST_TOO_FEW, as before).  The three are checked before anything else and
        otherwise ignored without polish=True.
        polish_cov=True (refused without polish=True): the polish call also returns the covariance of every polished pose (bundle_adjust_ragged(...,
        cov=True)), as cov_polished (S,12,12) and sigma0_polished (S,): NaN for a scene without a pose or with three or fewer matches in the polish.
        Every other key keeps its bits, and the device path still makes no synchronisation."""
        how = self._check_polish(polish_loss, polish_scale, polish_all, threshold, polish, polish_cov)
        adaptive = None if confidence is None else _check_adaptive(confidence, first_round)
        guided = self._check_guided(scenes, order, quality, growth)
        if refine is not None and refine not in RAGGED_METHODS:
            raise ValueError("robust_pose_scenes refines with one of %s, not %r" % (", ".join(RAGGED_METHODS), refine))
        if method not in ROBUST_METHODS:
            raise ValueError("robust_pose_scenes draws its hypotheses with LinearTFTPoseEstimation or LinearFPoseEstimation, not %r" % (method,))
        mid = METHOD_IDS[method]
        ns = 0 if n_sample is None else int(n_sample)
        args = (int(seed) & 0xFFFFFFFFFFFFFFFF, int(n_hyp), ns, float(threshold), int(candidates), int(lo_rounds))
        if isinstance(scenes, np.ndarray):
            sc = np.ascontiguousarray(scenes, dtype=np.float64)
            if sc.ndim != 2 or sc.shape[1] != 6:
                raise ValueError("scenes must be (Ntot, 6)")
            check_offsets(offsets)
            offsets = np.ascontiguousarray(offsets, dtype=np.int64)
            S = offsets.shape[0] - 1
            if offsets[-1] > sc.shape[0]:
                raise ValueError("offsets[-1] = %d beyond the %d packed correspondences" % (offsets[-1], sc.shape[0]))
            calm_cm, stride = self._calm_cm_np(calm, S)
            ranking = None
            if guided is not None:
                rank = guided[1] if guided[0] == "order" else order_from_quality(guided[1], offsets)
                ranking = (np.ascontiguousarray(rank, dtype=np.int32) if rank.shape[0] else np.zeros(1, dtype=np.int32), guided[2])
            assert int(offsets[-1]) <= sc.shape[0]
            out = self._robust_scenes_call(None, mid, sc, offsets, (), S, calm_cm, stride, args, adaptive, ranking)
            if getattr(self, "_score", 0):
                sco = self.inlier_count_scenes(sc, offsets, calm, out["R_t_2"], out["R_t_3"], threshold).cpu().numpy() if S else np.zeros(0, dtype=np.int32)
                out["score"] = np.where(out["status"] == 0, sco, -1).astype(np.int32)
            if refine is not None:
                keep = out["mask"] != 0
                inl = np.ascontiguousarray(sc[keep])
                cum = np.concatenate([[0], np.cumsum(keep, dtype=np.int64)])
                self._refined(out, self.pose_batch_ragged(refine, inl, cum[offsets], calm, reconst=False))
            return self._polish(out, calm, sc, offsets, False, how) if polish else out
        if not (isinstance(scenes, torch.Tensor) and scenes.is_cuda and scenes.dtype == torch.float64 and scenes.is_contiguous() and scenes.dim() == 2
                and scenes.shape[1] == 6):
            raise ValueError("scenes must be a contiguous float64 CUDA tensor of shape (Ntot, 6)")
        dev = scenes.device
        if not (isinstance(offsets, torch.Tensor) and offsets.is_cuda and offsets.device == dev and offsets.dtype == torch.int64 and offsets.dim() == 1
                and offsets.shape[0] >= 1):
            raise ValueError("offsets must be a 1-D int64 tensor of S + 1 entries on the device of scenes")
        offsets = offsets.contiguous()
        S = offsets.shape[0] - 1
        ntot = scenes.shape[0]
        calm_cm, stride = self._calm_scenes(calm, S, dev)
        if ns_max is None:                                                   # one synchronisation; pass ns_max to avoid it
            ns_max = max(0, int((offsets[1:] - offsets[:-1]).max().item())) if S > 0 else 0
        self.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        ranking = None
        if guided is not None:
            rank = guided[1]
            if guided[0] == "quality":                                       # stable sorts on the device: by descending quality, then by scene; nothing is read back
                q = torch.where(torch.isnan(rank), torch.full_like(rank, float("-inf")), rank).to(torch.float64)
                by_q = torch.argsort(-q, stable=True)
                scene = torch.searchsorted(offsets, torch.arange(ntot, dtype=torch.int64, device=dev), right=True) - 1   # -1 in front of offsets[0], S behind offsets[S]
                glob = by_q[torch.argsort(scene[by_q], stable=True)]
                sg = scene[glob]
                rank = torch.where((sg >= 0) & (sg < S), glob - offsets[sg.clamp(0, S)], torch.full_like(glob, -1)).to(torch.int32)
            ranking = (rank.contiguous() if ntot else torch.zeros(1, dtype=torch.int32, device=dev), guided[2])
        out = self._robust_scenes_call(dev, mid, scenes, offsets, (ntot, int(ns_max)), S, calm_cm, stride, args, adaptive, ranking)
        st = out["status"]
        if getattr(self, "_score", 0):                                       # one more count call on the returned poses; no pose (NaN): -1
            sco = self.inlier_count_scenes(scenes, offsets, calm, out["R_t_2"], out["R_t_3"], threshold) if S else torch.zeros_like(st)
            out["score"] = torch.where(st == 0, sco, torch.full_like(sco, -1))
        if refine is not None:
            # every scene's inliers first, in scene order, without reading a count: a stable sort of 1 - mask; all Ntot rows are kept, the offsets say
            # where the inliers end (boolean indexing and nonzero would synchronise)
            keep = (out["mask"] != 0).to(torch.int64)
            packed = scenes[torch.argsort(1 - keep, stable=True)]
            cum = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(keep, 0)])
            self._refined(out, self.pose_batch_ragged(refine, packed, cum[offsets.clamp(0, ntot)], calm, reconst=False, n_max=int(ns_max)))
        return self._polish(out, calm, scenes, offsets, False, how) if polish else out

    def inlier_count_scenes(self, scenes, offsets, calm, R_t_2, R_t_3, threshold=1.0):
        """Inlier counts of S * per_scene pose hypotheses against S packed scenes (tff_inlier_count_scenes_dev): R_t_2, R_t_3 (S * per_scene, 3, 4),
        hypothesis b against scene b // per_scene with its CalM ((9, 3) shared or (S, 9, 3)); what inlier_count gives per scene.  -> (S * per_scene,)
        int32 CUDA tensor, -1 for the hypotheses of a scene with bad offsets.  numpy offsets are validated (check_offsets) before the library is entered."""
        dev = torch.device("cuda", self.device)
        if isinstance(offsets, np.ndarray):
            check_offsets(offsets)
            offsets = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.int64))
        if not isinstance(offsets, torch.Tensor) or offsets.dim() != 1 or offsets.shape[0] < 1 or offsets.dtype != torch.int64:
            raise ValueError("offsets must be a 1-D int64 array or tensor of S + 1 entries")
        S = offsets.shape[0] - 1
        for name, a in (("scenes", scenes), ("R_t_2", R_t_2), ("R_t_3", R_t_3)):
            want = (6,) if name == "scenes" else (3, 4)
            if tuple(a.shape[1:]) != want:
                raise ValueError("%s must be (n, %s)" % (name, ", ".join(map(str, want))))
        B = R_t_2.shape[0]
        if R_t_3.shape[0] != B or (S == 0 and B != 0) or (S > 0 and B % S != 0):
            raise ValueError("R_t_2 and R_t_3 must hold the same multiple of S = %d poses" % S)
        if not isinstance(calm, (np.ndarray, torch.Tensor)) or tuple(calm.shape) not in ((9, 3), (S, 9, 3)):
            raise ValueError("CalM must be a (9, 3) or (S, 9, 3) array or tensor")
        self._begin()
        scenes = self._t(scenes); offsets = offsets.to(dev).contiguous()
        calm_cm, stride = self._calm_scenes(calm, S, dev)
        r2 = self._cams_cm(self._t(R_t_2)); r3 = self._cams_cm(self._t(R_t_3))
        cnt = torch.empty(B, dtype=torch.int32, device=dev)
        _check(self.lib, self.lib.tff_inlier_count_scenes_dev(self.handle, self._p(scenes), self._p(offsets), scenes.shape[0], S, self._p(calm_cm), stride,
                                                              self._p(r2), self._p(r3), B // S if S else 0, float(threshold), self._p(cnt)),
               "tff_inlier_count_scenes_dev")
        return cnt


class MultiContext:
    """A tff_multi: one process, one context + host thread + stream per device (include/tftfund.h, multi-GPU section).
    `devices`: list of HIP ordinals, or None for all visible devices."""

    def __init__(self, devices=None, lib_path=None):
        self.lib = load_library(lib_path)
        h = ctypes.c_void_p()
        if devices is None:
            arr, n = None, 0
        else:
            arr = (ctypes.c_int32 * len(devices))(*devices); n = len(devices)
        _check(self.lib, self.lib.tff_multi_create(ctypes.byref(h), arr, n), "tff_multi_create")
        self.handle = h
        self.size = int(self.lib.tff_multi_size(h))

    def shard(self, B, rank):
        b0, b1 = ctypes.c_int64(), ctypes.c_int64()
        self.lib.tff_multi_shard(self.handle, B, rank, ctypes.byref(b0), ctypes.byref(b1))
        return b0.value, b1.value

    def pose_batch(self, method, corresp, calm, reconst=True):
        """Host arrays in, host arrays out: corresp (B, N, 6), calm (9, 3) or (B, 9, 3); the shards run concurrently on the devices."""
        C = np.ascontiguousarray(corresp, dtype=np.float64)
        B, N, _ = C.shape
        calm = np.asarray(calm, dtype=np.float64)
        if calm.ndim == 2:
            cm, stride = np.ascontiguousarray(calm.T).reshape(27), 0
        else:
            cm, stride = np.ascontiguousarray(calm.transpose(0, 2, 1)).reshape(B, 27), 27
        Rt2 = np.empty((B, 12)); Rt3 = np.empty((B, 12)); T = np.empty((B, 27))
        Rec = np.empty((B, N, 3)) if reconst else None
        it = np.zeros(B, dtype=np.int32); st = np.zeros(B, dtype=np.int32)
        p = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None
        _check(self.lib, self.lib.tff_pose_batch_host_multi(self.handle, METHOD_IDS[method], p(C), p(cm), stride, B, N, p(Rt2), p(Rt3), p(T),
                                                            p(Rec), p(it), p(st)), "tff_pose_batch_host_multi")
        return dict(R_t_2=Rt2.reshape(B, 4, 3).transpose(0, 2, 1), R_t_3=Rt3.reshape(B, 4, 3).transpose(0, 2, 1),
                    T=T.reshape(B, 3, 3, 3).transpose(0, 3, 2, 1), Reconst=None if Rec is None else Rec.transpose(0, 2, 1), iter=it, status=st)

    def pose_batch_dev(self, method, corresp_shards, calm_shards, B):
        """Device-resident shards (torch CUDA tensors, shard g on device g, each (b1-b0, N, 6)); returns per device the gathered
        record tensor (G * chunk, 51) laid out as G blocks [Rt2 (chunk x 12) | Rt3 (chunk x 12) | T (chunk x 27)] and the status."""
        import torch
        G = self.size
        if B < 0 or len(corresp_shards) != G or len(calm_shards) != G:
            raise ValueError("pose_batch_dev needs B >= 0 and one shard per device")
        N = int(corresp_shards[0].shape[1])
        chunk = (B + G - 1) // G
        for g in range(G):
            b0, b1 = self.shard(B, g)
            c = corresp_shards[g]
            if c.dtype != torch.float64 or not c.is_contiguous() or tuple(c.shape) != (b1 - b0, N, 6):
                raise ValueError("shard %d must be a contiguous float64 tensor of shape (%d, %d, 6)" % (g, b1 - b0, N))
        recs = [torch.zeros(G * chunk * 51, dtype=torch.float64, device=corresp_shards[g].device) for g in range(G)]
        sts = [torch.zeros(G * chunk, dtype=torch.int32, device=corresp_shards[g].device) for g in range(G)]
        cms = [c.t().contiguous().reshape(27) for c in calm_shards]
        # torch enqueued the allocations / transposes above on ITS current stream of each device; the library works on each context's
        # stream.  Hand every context torch's stream of its device (tff_ctx_set_stream orders the hand-over with an event), so that
        # zero-fill -> kernels -> all-gather are one stream's program order and later torch work on the results is ordered too.
        for g in range(G):
            dev = corresp_shards[g].device
            _check(self.lib, self.lib.tff_ctx_set_stream(self.lib.tff_multi_ctx(self.handle, g), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                   "tff_ctx_set_stream")
        ptr = lambda ts: (ctypes.c_void_p * G)(*[t.data_ptr() for t in ts])
        _check(self.lib, self.lib.tff_pose_batch_dev_multi(self.handle, METHOD_IDS[method], ptr(corresp_shards), ptr(cms), 0, B, N, ptr(recs), ptr(sts)),
               "tff_pose_batch_dev_multi")
        for g in range(G):
            _check(self.lib, self.lib.tff_ctx_synchronize(self.lib.tff_multi_ctx(self.handle, g)), "synchronize")
        # everything is complete: give the borrowed torch streams back (a later call on these contexts -- pose_batch, another thread's
        # pose_batch_dev under a different torch stream -- must not run on a stream the caller may have destroyed meanwhile)
        for g in range(G):
            _check(self.lib, self.lib.tff_ctx_use_own_stream(self.lib.tff_multi_ctx(self.handle, g)), "tff_ctx_use_own_stream")
        return recs, sts, chunk

    def close(self):
        if getattr(self, "handle", None):
            self.lib.tff_multi_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx = threading.local()


def default_context(device=0):
    """One context per (thread, device): a context's workspaces are shared state, so threads do not share one."""
    d = getattr(_default_ctx, "by_device", None)
    if d is None:
        d = _default_ctx.by_device = {}
    c = d.get(device)
    if c is None:
        c = d[device] = Context(device)
    return c


def _single(method, Corresp, CalM, nargout=5):
    """One triplet with the reference's shapes: Corresp 6xN, CalM 9x3 ->
    R_t_2 (3x4), R_t_3 (3x4), Reconst (3xN), T (3x3x3), iter."""
    Corresp = np.asarray(Corresp, dtype=np.float64)
    if Corresp.ndim != 2 or Corresp.shape[0] != 6:
        raise ValueError("Corresp must be 6xN")
    N = Corresp.shape[1]
    out = default_context().pose_batch(method, np.ascontiguousarray(Corresp.T).reshape(1, N, 6), np.asarray(CalM),
                                       reconst=nargout >= 3)
    st = int(out["status"][0])
    if st == ST_TOO_FEW:
        raise ValueError("not enough correspondences for %s (N=%d)" % (method, N))
    if st == ST_NO_POSE:
        raise RuntimeError("%s: no pose candidate with non-negative cheirality score" % method)
    if st == ST_NO_PARAM:
        raise ValueError("The minimal param could not be found")
    rec = out["Reconst"][0] if out["Reconst"] is not None else None
    return out["R_t_2"][0], out["R_t_3"][0], rec, out["T"][0], int(out["iter"][0])


def LinearTFTPoseEstimation(Corresp, CalM):
    """Drop-in for TFT_methods/LinearTFTPoseEstimation.m (same inputs/outputs)."""
    return _single("LinearTFTPoseEstimation", Corresp, CalM)


def LinearFPoseEstimation(Corresp, CalM):
    """Drop-in for F_methods/LinearFPoseEstimation.m (same inputs/outputs; needs N >= 8)."""
    return _single("LinearFPoseEstimation", Corresp, CalM)


def ResslTFTPoseEstimation(Corresp, CalM):
    """Drop-in for TFT_methods/ResslTFTPoseEstimation.m (iter = Gauss-Helmert iterations)."""
    return _single("ResslTFTPoseEstimation", Corresp, CalM)


def FaugPapaTFTPoseEstimation(Corresp, CalM):
    """Drop-in for TFT_methods/FaugPapaTFTPoseEstimation.m (iter = Gauss-Helmert iterations)."""
    return _single("FaugPapaTFTPoseEstimation", Corresp, CalM)


def NordbergTFTPoseEstimation(Corresp, CalM):
    """Drop-in for TFT_methods/NordbergTFTPoseEstimation.m (iter = Gauss-Helmert iterations)."""
    return _single("NordbergTFTPoseEstimation", Corresp, CalM)


def OptimFPoseEstimation(Corresp, CalM):
    """Drop-in for F_methods/OptimFPoseEstimation.m (iter = it1 + it2 Gauss-Helmert iterations of the two optimF calls)."""
    return _single("OptimFPoseEstimation", Corresp, CalM)


def PiPoseEstimation(Corresp, CalM):
    """Drop-in for TFT_methods/PiPoseEstimation.m (iter = Gauss-Helmert iterations)."""
    return _single("PiPoseEstimation", Corresp, CalM)


def PiColPoseEstimation(Corresp, CalM):
    """Drop-in for TFT_methods/PiColPoseEstimation.m (collinear camera centres; iter = Gauss-Helmert iterations)."""
    return _single("PiColPoseEstimation", Corresp, CalM)


def _check_tracks_loss(missing, loss, scale):
    """loss= / scale= of bundle_adjust_views and BundleAdjustment: ValueError before a device is touched"""
    if loss is None:
        return
    if not isinstance(loss, str) or loss not in LOSS_IDS:
        raise ValueError('loss must be None, "huber" or "cauchy"')
    if missing != "point":
        raise ValueError('a loss needs missing="point": the whole-view call has none')
    if scale is None or isinstance(scale, bool) or not isinstance(scale, (int, float, np.integer, np.floating)) or not (0.0 < float(scale) < float("inf")):
        raise ValueError("a loss needs a positive finite scale (pixels)")


def BundleAdjustment(CalM, R_t_0, Corresp, Reconst0=None, missing="view", loss=None, scale=None):
    """Drop-in for Optimization/BundleAdjustment.m, M = 2 .. 6 views: CalM 3Mx3, R_t_0 3Mx4, Corresp 2MxN (NaN = not seen), Reconst0 3xN or None
    -> R_t (3Mx4, first camera [I|0], |t2| = 1), Reconst (3xN), iter, repr_err.  The initial triangulation (:59-77), the change of coordinates to
    camera 1 (:80-86) and the `isnan` branch (:165 -- it drops a whole VIEW, see csrc/ba_views_kernel.h) run on the device as the reference orders them.
    Raises ValueError where the reference stops with an error (fewer than two complete views to triangulate from, :73-74).
    missing="point": what the reference's header documents instead (:4-22; include/tftfund_tracks.h) -- a NaN means that this point is not seen in this
    view; a point seen in fewer than two views is dropped and its column of Reconst is NaN.  Raises ValueError when no point is seen in two views or a
    view's normalisation is not finite (a view with a single observation).
    loss="huber" | "cauchy", scale in pixels (missing="point" only; include/tftfund_tracks_loss.h): a robust loss per observation; repr_err is then
    sqrt(sum rho) in pixels."""
    if missing not in ("view", "point"):
        raise ValueError('missing must be "view" or "point"')
    _check_tracks_loss(missing, loss, scale)
    CalM = np.asarray(CalM, dtype=np.float64); R_t_0 = np.asarray(R_t_0, dtype=np.float64); Corresp = np.asarray(Corresp, dtype=np.float64)
    if Corresp.ndim != 2 or Corresp.shape[0] % 2 or not 2 <= Corresp.shape[0] // 2 <= 6:
        raise ValueError("Corresp must be 2M x N with M = 2 .. 6 views")
    M = Corresp.shape[0] // 2
    if R_t_0.shape != (3 * M, 4) or CalM.shape != (3 * M, 3):
        raise ValueError("%d views: R_t_0 must be %dx4 and CalM %dx3" % (M, 3 * M, 3 * M))
    X0 = None if Reconst0 is None else np.asarray(Reconst0, dtype=np.float64)[None]
    if missing == "point":
        if X0 is not None and X0.shape != (1, 3, Corresp.shape[1]):
            raise ValueError("Reconst0 must be 3 x N")
        out = default_context().bundle_adjust_views(CalM, R_t_0[None], np.ascontiguousarray(Corresp.T)[None], X0, missing="point", loss=loss, scale=scale)
        if int(out["status"][0]) == 1:
            raise ValueError("no point is seen in two views")
        if int(out["used"][0]) > 0 and bool(torch.isnan(out["R_t"][0]).all()):
            raise ValueError("a view's normalisation is not finite (Normalize2Ddata.m:35-37: a single observation, or coincident ones)")
        return out["R_t"][0].cpu().numpy(), out["Reconst"][0].cpu().numpy(), int(out["iter"][0]), float(out["repr_err"][0])
    out = default_context().bundle_adjust_views(CalM, R_t_0[None], np.ascontiguousarray(Corresp.T)[None], X0)
    if int(out["status"][0]) == 1:
        raise ValueError("fewer than two complete views: triangulation3D returns nothing (triangulation3D.m:36-38) and BundleAdjustment.m:73-74 stops")
    return out["R_t"][0].cpu().numpy(), out["Reconst"][0].cpu().numpy(), int(out["iter"][0]), float(out["repr_err"][0])
