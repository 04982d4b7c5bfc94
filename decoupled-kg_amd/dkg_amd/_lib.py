"""ctypes binding of ``libdkg.so`` (C ABI in ``include/dkg.h``).

The library is the product: there is no CPU fallback.  Loading fails loudly
when the shared object is missing, and every entry point raises on a non-zero
status with the library's own message.
"""

from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_size_t, c_uint, c_void_p

from .errors import BotorchTensorDimensionError, DkgNativeError, NotPSDError, UnsupportedError

# DKG_LIB: an alternative build of the same library (A/B measurements by tools/; never set in production)
LIB_PATH = os.environ.get("DKG_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "_native",
                                                     "libdkg.so")

ABI_VERSION = 9
DKG_XARG_MAX = 64  # include/dkg.h: largest B * d of dkg_plan_forward_grad_hostx
DKG_PLAN_GRAD = 1
DKG_PLAN_FORCE_WALK = 2  # test hook: envelope overflow path for every pair
DKG_PLAN_F32 = 4  # fp32 contractions (BASELINE configs[4]); forward only
DKG_PLAN_FUSED = 8  # the forward as one launch with in-launch hand-offs (dkg_fused.h); not the default
DKG_PLAN_NO_CHAIN = 16  # test hook: the streaming envelope's list-overflow path (no sample chain) for every pair
DKG_PLAN_GRAD_GLOBAL_ROWS = 32  # with GRAD: read the Q_X / J rows from the workspace where they do not fit in LDS
DKG_PLAN_FORCE_GLOBAL_ROWS = 128  # test hook, with GRAD: the streaming global-rows envelope on any shape
# dkg_debug_cov_kernels: the opt-in fp64 covariance block kernels (same bits as the defaults)
DKG_COV_ENABLE_BLK, DKG_COV_ENABLE_REC2, DKG_COV_ENABLE_REG = 1, 2, 4
MAX_OUTPUTS = 8
MAX_DIM = 16
# include/dkg.h: the limits of the joint entropy search plan (dkg_jes_init)
DKG_JES_MAX_SAMPLES, DKG_JES_MAX_BOXES, DKG_JES_MAX_CANDIDATES = 64, 4096, 65536
# include/dkg.h: the limits of the hypervolume knowledge gradient plan (dkg_hvkg_init)
DKG_HVKG_MAX_FANTASIES, DKG_HVKG_MAX_PARETO, DKG_HVKG_MAX_RESTARTS = 64, 32, 4096
# include/dkg.h: the limits of dkg_dominated_boxes and dkg_hypervolume_front
DKG_BOXES_MAX_POINTS, DKG_HV_FRONT_MAX_POINTS = 2048, 16384

(DKG_OK, DKG_ERR_ARG, DKG_ERR_UNSUPPORTED, DKG_ERR_WORKSPACE, DKG_ERR_HIP, DKG_ERR_NO_LINES,
 DKG_ERR_NOT_PD) = range(7)


class DkgOutput(ctypes.Structure):
    """``struct dkg_output`` (include/dkg.h)."""

    _fields_ = [
        ("n", c_int32),
        ("kernel", c_int32),
        ("outputscale", c_double),
        ("noise", c_double),
        ("mean_constant", c_double),
        ("y_mean", c_double),
        ("y_std", c_double),
        ("inv_lengthscale", c_void_p),
        ("train_x", c_void_p),
        ("alpha", c_void_p),
        ("root_frag", c_void_p),
        ("disc_frag", c_void_p),
        ("disc_mean", c_void_p),
    ]


class DkgNsga2Params(ctypes.Structure):
    """``struct dkg_nsga2_params`` (include/dkg.h); the defaults are pygmo.nsga2's documented ones."""

    _fields_ = [("cr", c_double), ("eta_c", c_double), ("m", c_double), ("eta_m", c_double),
                ("raw_inputs", c_int32), ("reserved", c_int32)]

    def __init__(self, cr=0.95, eta_c=10.0, m=0.01, eta_m=50.0, raw_inputs=0):
        super().__init__(cr, eta_c, m, eta_m, int(raw_inputs), 0)


DKG_RFF_MAX_FEATURES = 1024  # include/dkg.h: random Fourier features per path


class DkgRffPaths(ctypes.Structure):
    """``struct dkg_rff_paths`` (include/dkg.h): S sample paths of an m-output model."""

    _fields_ = [("S", c_int32), ("m", c_int32), ("d", c_int32), ("R", c_int32), ("omega", c_void_p),
                ("bias", c_void_p), ("coef", c_void_p), ("offset", c_void_p)]


DKG_APPEND_MAX_ROWS, DKG_APPEND_MAX_JOBS = 32, 512  # include/dkg.h: the limits of dkg_append_rows


class DkgAppendJob(ctypes.Structure):
    """``struct dkg_append_job`` (include/dkg.h): one (state, output) of a ``dkg_append_rows`` call."""

    _fields_ = [("o", POINTER(DkgOutput)), ("L", c_void_p), ("Linv", c_void_p), ("disc", c_void_p), ("N", c_int32),
                ("K", c_int32), ("train_x", c_void_p), ("train_y", c_void_p), ("jitter", c_double),
                ("L_new", c_void_p), ("Linv_new", c_void_p), ("alpha_new", c_void_p), ("root_frag_new", c_void_p),
                ("disc_frag_new", c_void_p), ("disc_mean_new", c_void_p)]


# name -> (restype, argtypes); every symbol include/dkg.h declares.
SIGNATURES = {
    "dkg_append_rows_workspace": (c_size_t, [POINTER(DkgAppendJob), c_int, c_int]),
    "dkg_append_rows": (c_int, [POINTER(DkgAppendJob), c_int, c_int, POINTER(c_int32), c_void_p, c_size_t, c_void_p]),
    "dkg_rff_workspace": (c_size_t, [c_int, c_int]),
    "dkg_rff_weights": (c_int, [POINTER(DkgOutput), c_int, c_int, POINTER(c_void_p), c_void_p, c_void_p, c_void_p,
                                c_void_p, c_int, POINTER(DkgRffPaths), c_void_p, c_size_t, POINTER(c_double),
                                c_void_p]),
    "dkg_debug_rff_gram": (c_int, [c_int]),
    "dkg_rff_eval": (c_int, [POINTER(DkgRffPaths), c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "dkg_pareto_paths_workspace": (c_size_t, [c_int, c_int, c_int, c_int]),
    "dkg_pareto_nsga2_paths": (c_int, [POINTER(DkgRffPaths), c_void_p, c_void_p, c_int, c_int,
                                       POINTER(DkgNsga2Params), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_size_t, c_void_p]),
    "dkg_pareto_prune": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "dkg_posterior_mean": (c_int, [POINTER(DkgOutput), c_int, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "dkg_pareto_rank": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                c_void_p]),
    "dkg_pareto_rank_workspace": (c_size_t, [c_int, c_int]),
    "dkg_debug_pareto_wide": (c_int, [c_int]),
    "dkg_pareto_draws": (c_size_t, [c_int, c_int]),
    "dkg_pareto_variation": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                     POINTER(DkgNsga2Params), c_void_p, c_void_p, c_void_p]),
    "dkg_pareto_workspace": (c_size_t, [c_int, c_int, c_int]),
    "dkg_pareto_nsga2": (c_int, [POINTER(DkgOutput), c_int, c_int, c_void_p, c_void_p, c_int, c_int,
                                 POINTER(DkgNsga2Params), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_size_t, c_void_p]),
    "dkg_jes_plan_bytes": (c_size_t, []),
    "dkg_jes_workspace": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "dkg_jes_init": (c_int, [POINTER(DkgOutput), c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p,
                             c_size_t, c_void_p, c_void_p]),
    "dkg_jes_forward": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dkg_hvkg_plan_bytes": (c_size_t, []),
    "dkg_hvkg_workspace": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "dkg_hvkg_init": (c_int, [POINTER(DkgOutput), c_int, c_int, POINTER(c_double), c_int, c_int, POINTER(c_double),
                              c_uint, c_double, c_double, c_int, c_void_p, c_size_t, c_void_p, c_void_p]),
    "dkg_hvkg_forward": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dkg_hypervolume": (c_int, [c_void_p, c_int, c_int, c_int, POINTER(c_double), c_void_p, c_void_p, c_void_p]),
    "dkg_dominated_boxes_workspace": (c_size_t, [c_int, c_int, c_int]),
    "dkg_dominated_boxes": (c_int, [c_void_p, c_int, c_int, c_int, POINTER(c_double), c_int, c_void_p, c_void_p,
                                    c_void_p, c_size_t, c_void_p]),
    "dkg_hypervolume_front_workspace": (c_size_t, [c_int, c_int, c_int]),
    "dkg_hypervolume_front": (c_int, [c_void_p, c_int, c_int, c_int, POINTER(c_double), c_void_p, c_void_p, c_size_t,
                                      c_void_p]),
    "dkg_abi_version": (c_int, []),
    "dkg_last_error": (c_char_p, []),
    "dkg_frag_elems": (c_size_t, [c_int, c_int]),
    "dkg_kernel_matrix": (c_int, [POINTER(DkgOutput), c_int, c_void_p, c_int, c_void_p, c_int, c_double,
                                  c_void_p, c_void_p]),
    "dkg_pack_root": (c_int, [c_void_p, c_int, c_void_p, c_void_p]),
    "dkg_prepare_workspace": (c_size_t, [c_int]),
    "dkg_prepare_output": (c_int, [POINTER(DkgOutput), c_int, c_void_p, c_int, c_void_p, c_void_p, c_size_t,
                                   c_void_p, c_void_p, POINTER(c_double), c_void_p]),
    "dkg_prepare_outputs": (c_int, [POINTER(DkgOutput), c_int, c_int, POINTER(c_void_p), c_int, POINTER(c_void_p),
                                    POINTER(c_void_p), POINTER(c_size_t), POINTER(c_void_p), POINTER(c_void_p),
                                    POINTER(c_double), c_void_p]),
    "dkg_cross_root": (c_int, [POINTER(DkgOutput), c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "dkg_append_workspace": (c_size_t, [c_int, c_int]),
    "dkg_append_observation": (c_int, [POINTER(DkgOutput), c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                       c_void_p, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_size_t, c_void_p]),
    "dkg_mll_workspace": (c_size_t, [POINTER(c_int), c_int]),
    "dkg_mll_value_grad": (c_int, [POINTER(DkgOutput), c_int, c_int, POINTER(c_void_p), c_int, c_void_p, c_size_t,
                                   POINTER(c_double), POINTER(c_double), POINTER(c_double), c_void_p]),
    "dkg_forward_workspace": (c_size_t, [POINTER(DkgOutput), c_int, c_int, c_int, c_int]),
    "dkg_forward": (c_int, [POINTER(DkgOutput), c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int,
                            c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "dkg_forward_timed": (c_int, [POINTER(DkgOutput), c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                  c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p,
                                  POINTER(c_float)]),
    "dkg_plan_bytes": (c_size_t, []),
    "dkg_plan_workspace": (c_size_t, [POINTER(DkgOutput), c_int, c_int, c_int, c_int, c_int, c_int]),
    "dkg_plan_init": (c_int, [POINTER(DkgOutput), c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int,
                              c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]),
    "dkg_plan_workspace_targets": (c_size_t, [POINTER(DkgOutput), c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "dkg_plan_init_targets": (c_int, [POINTER(DkgOutput), c_int, c_int, c_void_p, c_int, c_void_p, c_int,
                                      POINTER(c_int), c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p,
                                      c_void_p]),
    "dkg_plan_forward_grad": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "dkg_plan_forward_grad_hostx": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                            c_void_p, c_void_p]),
    "dkg_plan_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "dkg_plan_forward_batches": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "dkg_plan_forward_timed": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                       POINTER(c_float)]),
    "dkg_plan_time_stage": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int,
                                    c_int, POINTER(c_float)]),
    "dkg_plan_time_stage_batches": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int,
                                            c_int, POINTER(c_float)]),
    "dkg_plan_hull_sizes": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    "dkg_plan_status": (c_int, [c_void_p, POINTER(c_int), c_int, c_void_p]),
    "dkg_plan_fused": (c_int, [c_void_p]),
    "dkg_plan_grad_rows": (c_int, [POINTER(DkgOutput), c_int, c_int, c_int, c_int, c_int]),
    "dkg_plan_grad_rows_of": (c_int, [c_void_p]),
    "dkg_lines_kg": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "dkg_epigraph": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dkg_pwl_expectation": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "dkg_plan_lines": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "dkg_launcher_create": (c_int, [c_int, POINTER(c_void_p)]),
    "dkg_launcher_arm": (c_int, [c_void_p, c_double]),
    "dkg_launcher_graphs": (c_int, [c_void_p, c_int, POINTER(c_void_p), POINTER(c_int), POINTER(c_void_p)]),
    "dkg_launcher_destroy": (c_int, [c_void_p]),
    "dkg_debug_read_kstamps": (c_int, [c_void_p, c_int]),
    "dkg_debug_wave_ops": (c_int, [c_void_p, c_void_p, c_void_p]),
    "dkg_debug_cov_kernels": (c_int, [c_int]),
    "dkg_debug_cross_tall": (c_int, [c_int]),
    "dkg_debug_cross_tall_launches": (ctypes.c_longlong, []),
    "dkg_debug_cross_tall_eligible": (c_int, [c_int, c_int, c_int, c_int]),
    "dkg_debug_plan_envelope": (c_int, [c_void_p, POINTER(c_int)]),
    "dkg_debug_plan_qx32": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "dkg_debug_f32_dispatch": (c_int, [c_int] * 6 + [POINTER(c_int)]),
    "dkg_debug_mfma_f64": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "dkg_debug_envelope_lds": (c_int, [c_int] * 9 + [POINTER(c_int)]),
    "dkg_debug_envelope_deal": (c_int, [c_int] * 3 + [POINTER(c_int)] * 2),
}

_lib = None


def load() -> ctypes.CDLL:
    """Load and type the native library once (raises DkgNativeError if absent)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DkgNativeError(
            f"libdkg.so not found at {LIB_PATH}; build it with `make -C decoupled-kg_amd` "
            f"(or __graft_entry__.build()).  There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.dkg_abi_version() != ABI_VERSION:
        raise DkgNativeError(f"libdkg.so ABI {lib.dkg_abi_version()} != expected {ABI_VERSION}; rebuild it")
    _lib = lib
    return lib


def check(status: int, what: str) -> None:
    if status == DKG_OK:
        return
    msg = f"{what}: {load().dkg_last_error().decode(errors='replace')}"
    if status == DKG_ERR_ARG:
        raise BotorchTensorDimensionError(msg)
    if status == DKG_ERR_UNSUPPORTED:
        if "gradient:" in msg and "envelope stage's LDS" in msg:
            msg += '. dkg_amd.set_gradient_rows("auto") builds a plan that reads those rows from global memory instead.'
        raise UnsupportedError(msg)
    if status == DKG_ERR_NO_LINES:
        raise ValueError(msg)
    if status == DKG_ERR_NOT_PD:
        raise NotPSDError(msg)
    raise DkgNativeError(msg)


def check_fit(status: int, what: str) -> None:
    """``check`` for the fit's objective (dkg_mll_value_grad): a covariance that is not positive definite after
    the jitter retries raises the ``torch.linalg.LinAlgError`` the host objective's ``fit._chol`` raises."""
    if status == DKG_ERR_NOT_PD:
        import torch

        raise torch.linalg.LinAlgError(f"{what}: {load().dkg_last_error().decode(errors='replace')}")
    check(status, what)


def ptr(t) -> int:
    """Device address of a tensor (0 for None)."""
    return 0 if t is None else int(t.data_ptr())
