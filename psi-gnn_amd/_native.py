"""ctypes binding of libpsignn_hip.so (C ABI declared in include/psignn_hip.h).

There is no CPU fallback: if the shared library is missing or a call fails, an exception is
raised.  Tensors cross the boundary as raw device pointers (``tensor.data_ptr()``) on the
current HIP stream; torch only supplies memory and streams.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpsignn_hip.so")

D = 10   # the default latent width: libpsignn_hip.so, every entry point
# Other widths: libpsignn_hip_d<w>.so, the forward translation units built once more with -DPSIGNN_D=<w> (csrc/Makefile).  They
# hold forward inference only -- f, the solvers that need only f -- and ``lib(w)`` binds what they export.
SUPPORTED_WIDTHS = (8, 10, 16)


def lib_path(width: int = D) -> str:
    return LIB_PATH if width == D else os.path.join(_HERE, f"libpsignn_hip_d{int(width)}.so")


def check_width(width) -> int:
    """``width`` as an int if a library is built for it, NativeError naming the supported widths otherwise."""
    try:
        ok = int(width) == width and int(width) in SUPPORTED_WIDTHS
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise NativeError(f"latent_dim {width!r} is not supported: the HIP kernels are built for latent_dim in {SUPPORTED_WIDTHS} "
                          f"({D}: everything; the others: forward inference only)")
    return int(width)


def forward_only_error(width, what) -> "NativeError":
    return NativeError(f"{what}: latent_dim {width} has forward inference only (f, the encoder / decoder and the solvers that need "
                       f"only f); derivatives, training and the baselines exist at latent_dim {D}")


def require_default_width(width, what):
    """Raise the "forward inference only" error unless ``width`` is the default one.  Host side, before any native call."""
    if int(width) != D:
        raise forward_only_error(width, what)


class NativeError(RuntimeError):
    pass


class SolveInfo(C.Structure):
    _fields_ = [("nstep", C.c_int32), ("n_iter", C.c_int32), ("prot_break", C.c_int32),
                ("stop_reason", C.c_int32), ("lowest", C.c_double), ("lowest_abs", C.c_double)]


class GmresAdjointInfo(C.Structure):
    _fields_ = [("products", C.c_int32), ("cycles", C.c_int32), ("stop_reason", C.c_int32), ("n_reorth", C.c_int32),
                ("lowest", C.c_double), ("lowest_abs", C.c_double)]


class Gmres64Opts(C.Structure):
    _fields_ = [("augment", C.c_int32), ("stall", C.c_double)]


class Gmres64Info(C.Structure):
    _fields_ = [("products", C.c_int32), ("cycles", C.c_int32), ("stop_reason", C.c_int32), ("n_reorth", C.c_int32),
                ("lowest", C.c_double), ("lowest_abs", C.c_double), ("n_aug", C.c_int32)]


class GmresOpts(C.Structure):   # psignn_gmres_opts_t
    _fields_ = [("augment", C.c_int32), ("stall", C.c_double)]


class GmresInfo(C.Structure):   # psignn_gmres_info_t
    _fields_ = [("products", C.c_int32), ("cycles", C.c_int32), ("stop_reason", C.c_int32), ("n_reorth", C.c_int32),
                ("lowest", C.c_double), ("lowest_abs", C.c_double), ("n_aug", C.c_int32)]


class Newton64Opts(C.Structure):
    _fields_ = [("eps", C.c_double), ("sigma0", C.c_double), ("eta", C.c_double), ("growth", C.c_double), ("reject_floor", C.c_double),
                ("sigma_off", C.c_double), ("threshold", C.c_int32), ("max_products", C.c_int32), ("max_rejects", C.c_int32),
                ("poll_every", C.c_int32)]


class Newton64Info(C.Structure):
    _fields_ = [("nstep", C.c_int32), ("n_iter", C.c_int32), ("n_accepted", C.c_int32), ("n_products", C.c_int32),
                ("n_feval", C.c_int32), ("stop_reason", C.c_int32), ("lowest", C.c_double), ("lowest_abs", C.c_double)]


class CgInfo(C.Structure):
    _fields_ = [("n_iter", C.c_int32), ("converged", C.c_int32), ("rel", C.c_double), ("true_rel", C.c_double),
                ("b_norm", C.c_double), ("sym_defect", C.c_double)]


_P = C.c_void_p
_I64 = C.c_int64
_INT = C.c_int

# name -> (restype, argtypes); mirrors include/psignn_hip.h one to one
SIGNATURES = {
    "psignn_last_error": (C.c_char_p, []),
    "psignn_version": (_INT, []),
    "psignn_latent_dim": (_INT, []),
    "psignn_plan_create": (_INT, [C.POINTER(_P), _I64, _I64, _P, _P, _P, _P, _INT, _P, _INT, _P]),
    "psignn_plan_is_tiled": (_INT, [_P]),
    "psignn_plan_num_tiles": (_I64, [_P]),
    "psignn_plan_ell_rows": (_I64, [_P]),
    "psignn_plan_max_tile_rows": (_INT, [_P]),
    "psignn_plan_permute": (_INT, [_P, _P, _INT, _P, _INT, _P]),
    "psignn_f_forward_p": (_INT, [_P, _P, _INT, _P, _P, _P, _P, _P, _P, _P]),
    "psignn_picard_p": (_INT, [_P, _P, _INT, _P, _P, _P, _P, _P, _P, _INT, _P]),
    "psignn_plan_destroy": (None, [_P]),
    "psignn_plan_num_nodes": (_I64, [_P]),
    "psignn_plan_num_edges": (_I64, [_P]),
    "psignn_plan_num_nonself_edges": (_I64, [_P]),
    "psignn_plan_export": (_INT, [_P, _INT, _P, C.c_size_t]),
    "psignn_weights_size": (_I64, [_INT, _INT]),
    "psignn_f_workspace_floats": (_I64, [_P]),
    "psignn_f_forward": (_INT, [_P, _P, _INT, _P, _P, _P, _P, _P, _P, _P]),
    "psignn_phi": (_INT, [_P, _P, _INT, _INT, _INT, _P, _P, _P, _P]),
    "psignn_f_jvp": (_INT, [_P, _P, _INT, _P, _P, _P, _P, _P, _P, _P]),
    "psignn_f_jvp_p": (_INT, [_P, _P, _INT, _P, _P, _P, _P, _P, _P]),
    "psignn_f_jvp_pw": (_INT, [_P, _P, _INT, _P, _P, _P, _P, _P, _P, _P]),
    "psignn_f_param_vjp_ex": (_INT, [_P, _P, _INT, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "psignn_f_layers_workspace_floats": (_I64, [_P, _INT]),
    "psignn_lin_create": (_INT, [_P, _P]),
    "psignn_lin_destroy": (None, [_P]),
    "psignn_lin_bytes": (C.c_size_t, [_P]),
    "psignn_lin_build": (_INT, [_P, _P, _INT, _P, _P, _P, _P]),
    "psignn_lin_jvp": (_INT, [_P, _P, _INT, _P, _P, _P]),
    "psignn_lin_vjp": (_INT, [_P, _P, _INT, _P, _P, _P, _P]),
    "psignn_lin_create_opts": (_INT, [_P, _P, _INT]),
    "psignn_lin_neumann_stored": (_INT, [_P]),
    "psignn_f_vjp": (_INT, [_P, _P, _INT, _P, _P, _P, _P, _P, _P, _P]),
    "psignn_f_vjp_p": (_INT, [_P, _P, _INT, _P, _P, _P, _P, _P, _P, _P]),
    "psignn_param_grad_size": (_I64, [_INT, _INT]),
    "psignn_f_param_vjp_workspace_floats": (_I64, [_P]),
    "psignn_f_param_vjp": (_INT, [_P, _P, _INT, _P, _P, _P, _P, _P, _P, _P, _P]),
    "psignn_f_param_vjp_p": (_INT, [_P, _P, _INT, _P, _P, _P, _P, _P, _P, _P]),
    "psignn_f_vjp_backward_workspace_floats": (_I64, [_P]),
    "psignn_f_vjp_backward": (_INT, [_P, _P, _INT, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "psignn_f_vjp_backward_tiled_ok": (_INT, [_P, _INT]),
    "psignn_f_vjp_backward_p_workspace_floats": (_I64, [_P]),
    "psignn_f_vjp_backward_p": (_INT, [_P, _P, _INT, _P, _P, _P, _P, _P, _P, _P, _P]),
    "psignn_mlp2_backward_workspace_floats": (_I64, [_I64]),
    "psignn_mlp2_backward": (_INT, [_P, _P, _I64, _INT, _INT, _INT, _P, _P, _P, _P, _P, _P, _P]),
    "psignn_residual_t": (_INT, [_P, _P, _P, _P, _P]),
    "psignn_dsgps_weights_size": (_I64, [_INT]),
    "psignn_dsgps_forward": (_INT, [_P, _P, _INT, _P, _P, _P, _P, _P, _P]),
    "psignn_dsgps_step_p": (_INT, [_P, _P, _P, _P, _P, _P, _P, _P]),
    "psignn_dsgps_grad_size": (_I64, [_INT]),
    "psignn_dsgps_step_backward_workspace_floats": (_I64, [_P]),
    "psignn_dsgps_step_backward": (_INT, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "psignn_dss_weights_size": (_I64, [_INT]),
    "psignn_dss_forward": (_INT, [_P, _P, _INT, C.c_float, _P, _P, _P, _P]),
    "psignn_dss_step_p": (_INT, [_P, _P, _INT, C.c_float, _P, _P, _P, _P]),
    "psignn_dss_grad_size": (_I64, []),
    "psignn_dss_step_backward_workspace_floats": (_I64, [_P]),
    "psignn_dss_step_backward": (_INT, [_P, _P, C.c_float, _P, _P, _P, _P, _P, _P, _P]),
    "psignn_mlp2": (_INT, [_P, _I64, _INT, _INT, _INT, _P, _P, _P, _P, _P, _P]),
    "psignn_residual": (_INT, [_P, _P, _P, _P, _P]),
    "psignn_broyden_create": (_INT, [C.POINTER(_P), _P, _INT, _INT]),
    "psignn_broyden_create_for_batch": (_INT, [C.POINTER(_P), _P, _INT, _INT, _I64]),
    "psignn_broyden_create_n": (_INT, [C.POINTER(_P), _I64, _INT, _INT, _INT]),
    "psignn_broyden_create_opts": (_INT, [C.POINTER(_P), _P, _I64, _INT, _INT, _INT, _I64, _INT]),
    "psignn_broyden_destroy": (None, [_P]),
    "psignn_broyden_bytes": (C.c_size_t, [_P]),
    "psignn_broyden_set_stop_mode": (_INT, [_P, _INT]),
    "psignn_broyden_solve": (_INT, [_P, _P, _INT, _P, _P, _P, C.c_double, _INT, _P, C.POINTER(SolveInfo),
                                    C.POINTER(C.c_double), C.POINTER(C.c_double), _P]),
    "psignn_broyden_solve_adjoint": (_INT, [_P, _P, _INT, _P, _P, _P, _P, C.c_double, _INT, _P, C.POINTER(SolveInfo),
                                            C.POINTER(C.c_double), C.POINTER(C.c_double), _P]),
    "psignn_broyden_solve_adjoint_lin": (_INT, [_P, _P, _P, _INT, _P, C.c_double, _INT, _P, C.POINTER(SolveInfo),
                                                C.POINTER(C.c_double), C.POINTER(C.c_double), _P]),
    "psignn_broyden_solve_batch": (_INT, [_INT, C.POINTER(_P), _P, _INT, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), C.c_double, _INT,
                                          C.POINTER(_P), C.POINTER(SolveInfo), C.POINTER(C.POINTER(C.c_double)),
                                          C.POINTER(C.POINTER(C.c_double)), _P]),
    "psignn_broyden_batchable": (_INT, [_INT, C.POINTER(_P)]),
    "psignn_broyden_solve_adjoint_lin_batch": (_INT, [_INT, C.POINTER(_P), C.POINTER(_P), _P, _INT, C.POINTER(_P), C.c_double, _INT,
                                               C.POINTER(_P), C.POINTER(SolveInfo), C.POINTER(C.POINTER(C.c_double)),
                                               C.POINTER(C.POINTER(C.c_double)), _P]),
    "psignn_broyden_adjoint_batchable": (_INT, [_INT, C.POINTER(_P), C.POINTER(_P)]),
    "psignn_broyden_get_iterate": (_INT, [_P, _INT, _P, _P]),
    "psignn_broyden_get_pair": (_INT, [_P, _INT, _INT, _P, _P]),
    "psignn_broyden_ext_begin": (_INT, [_P, _P, _P, _P]),
    "psignn_broyden_ext_next_x": (_INT, [_P, _P, _P]),
    "psignn_broyden_ext_trial_x": (_INT, [_P, C.c_double, _P, _P]),
    "psignn_broyden_ext_scale_step": (_INT, [_P, C.c_double, _P]),
    "psignn_broyden_ext_update": (_INT, [_P, _P, C.c_double, C.POINTER(_INT), _P]),
    "psignn_broyden_ext_finish": (_INT, [_P, _P, C.POINTER(SolveInfo), C.POINTER(C.c_double),
                                         C.POINTER(C.c_double), _P]),
    "psignn_fpiter_create": (_INT, [C.POINTER(_P), _I64, _INT, _INT, _INT]),
    "psignn_fpiter_destroy": (None, [_P]),
    "psignn_fpiter_bytes": (C.c_size_t, [_P]),
    "psignn_fpiter_poll": (_INT, [_P, C.POINTER(_INT), _P]),
    "psignn_picard_begin": (_INT, [_P, _P, _P]),
    "psignn_picard_current_x": (_INT, [_P, _P, _P]),
    "psignn_picard_update": (_INT, [_P, _P, C.c_double, C.POINTER(_INT), _P]),
    "psignn_anderson_begin": (_INT, [_P, _P, _P, _P, C.c_double, C.c_double, _INT, _P]),
    "psignn_anderson_next_x": (_INT, [_P, _P, _P]),
    "psignn_anderson_update": (_INT, [_P, _P, C.c_double, C.POINTER(_INT), _P]),
    "psignn_fpiter_finish": (_INT, [_P, _P, C.POINTER(SolveInfo), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                    C.POINTER(C.c_int32), _P]),
    "psignn_fpiter_get_iterate": (_INT, [_P, _INT, _P, _P]),
    "psignn_fpiter_create_for_batch": (_INT, [C.POINTER(_P), _I64, _INT, _INT, _INT, _I64]),
    "psignn_fpiter_batchable": (_INT, [_INT, C.POINTER(_P), C.POINTER(_P)]),
    "psignn_anderson_solve_batch": (_INT, [_INT, C.POINTER(_P), C.POINTER(_P), _P, _INT, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P),
                                           C.c_double, C.c_double, _INT, C.c_double, _INT, C.POINTER(_P), C.POINTER(SolveInfo),
                                           C.POINTER(C.POINTER(C.c_double)), C.POINTER(C.POINTER(C.c_double)),
                                           C.POINTER(C.POINTER(C.c_int32)), _P]),
    "psignn_picard_solve_batch": (_INT, [_INT, C.POINTER(_P), C.POINTER(_P), _P, _INT, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P),
                                         C.c_double, _INT, C.POINTER(_P), C.POINTER(SolveInfo), C.POINTER(C.POINTER(C.c_double)),
                                         C.POINTER(C.POINTER(C.c_double)), _P]),
    "psignn_gmres_create": (_INT, [C.POINTER(_P), _I64, _I64, _INT, _P]),
    "psignn_gmres_destroy": (None, [_P]),
    "psignn_gmres_bytes": (C.c_size_t, [_P]),
    "psignn_residual_norms": (_INT, [_P, _P, _P, _P, _P, C.POINTER(C.c_double), _P]),
    "psignn_gmres_begin": (_INT, [_P, _P, _P]),
    "psignn_gmres_step": (_INT, [_P, _INT, C.c_double, C.c_double, C.POINTER(_INT), _P]),
    "psignn_gmres_solution": (_INT, [_P, _INT, _P, C.c_double, _P, C.POINTER(C.c_double), _P]),
    "psignn_gmres_history": (_INT, [_P, C.POINTER(C.c_double), _P]),
    "psignn_gmres_reorth_count": (_INT, [_P, C.POINTER(C.c_int), _P]),
    "psignn_gmres_adjoint_workspace_floats": (_I64, [_P, _INT]),
    "psignn_gmres_solve_adjoint": (_INT, [_P, _P, _P, _INT, _P, _P, _P, _P, C.c_double, _INT, _INT, _P, _P,
                                          C.POINTER(GmresAdjointInfo), C.POINTER(C.c_double), C.POINTER(C.c_double), _P]),
    "psignn_gmres_solve_adjoint_lin": (_INT, [_P, _P, _P, _INT, _P, C.c_double, _INT, _INT, _P, _P,
                                              C.POINTER(GmresAdjointInfo), C.POINTER(C.c_double), C.POINTER(C.c_double), _P]),
    "psignn_gmres_create_for_batch": (_INT, [C.POINTER(_P), _I64, _I64, _INT, _P, _I64]),
    "psignn_gmres_create_aug": (_INT, [C.POINTER(_P), _I64, _I64, _INT, _P, _INT, _P, _I64]),
    "psignn_gmres_solve_adjoint_opts": (_INT, [_P, _P, _P, _INT, _P, _P, _P, _P, C.c_double, _INT, _INT, C.POINTER(GmresOpts), _P, _P,
                                               C.POINTER(GmresInfo), C.POINTER(C.c_double), C.POINTER(C.c_double), _P]),
    "psignn_gmres_solve_adjoint_lin_opts": (_INT, [_P, _P, _P, _INT, _P, C.c_double, _INT, _INT, C.POINTER(GmresOpts), _P, _P,
                                                   C.POINTER(GmresInfo), C.POINTER(C.c_double), C.POINTER(C.c_double), _P]),
    "psignn_gmres_adjoint_batchable": (_INT, [_INT, C.POINTER(_P), C.POINTER(_P)]),
    "psignn_gmres_solve_adjoint_lin_batch": (_INT, [_INT, C.POINTER(_P), C.POINTER(_P), _P, _INT, C.POINTER(_P), C.c_double, _INT, _INT,
                                                    C.POINTER(_P), C.POINTER(_P), C.POINTER(GmresAdjointInfo),
                                                    C.POINTER(C.POINTER(C.c_double)), C.POINTER(C.POINTER(C.c_double)), _P]),
    "psignn_cg_create": (_INT, [C.POINTER(_P), _P, _P, _INT, _P]),
    "psignn_cg_destroy": (None, [_P]),
    "psignn_cg_solve": (_INT, [_P, _P, _INT, _P, C.c_double, _INT, _INT, _P, C.POINTER(CgInfo), C.POINTER(C.c_double), _P]),
    "psignn_f64_weights_size": (_I64, [_INT, _INT]),
    "psignn_f64_create": (_INT, [C.POINTER(_P), _P, _P, _INT, _P]),
    "psignn_f64_destroy": (None, [_P]),
    "psignn_f64_forward": (_INT, [_P, _P, _INT, _P, _P, _P, _P, _P, _P]),
    "psignn_mlp2_f64": (_INT, [_P, _I64, _INT, _INT, _INT, _P, _P, _P, _P, _P, _P]),
    "psignn_broyden64_create": (_INT, [C.POINTER(_P), _P, _INT]),
    "psignn_broyden64_destroy": (None, [_P]),
    "psignn_broyden64_bytes": (C.c_size_t, [_P]),
    "psignn_broyden64_solve": (_INT, [_P, _P, _INT, _P, _P, _P, _P, C.c_double, _INT, _P, C.POINTER(SolveInfo),
                                      C.POINTER(C.c_double), C.POINTER(C.c_double), _P]),
    "psignn_f64_deriv_workspace_doubles": (_I64, [_P, _INT, _INT]),
    "psignn_f64_jvp": (_INT, [_P, _P, _INT, _P, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "psignn_f64_vjp": (_INT, [_P, _P, _INT, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "psignn_broyden64_solve_adjoint": (_INT, [_P, _P, _INT, _P, _P, _P, _P, _P, C.c_double, _INT, _P, _I64, _P, C.POINTER(SolveInfo),
                                              C.POINTER(C.c_double), C.POINTER(C.c_double), _P]),
    "psignn_gmres64_create": (_INT, [C.POINTER(_P), _P, _INT]),
    "psignn_gmres64_destroy": (None, [_P]),
    "psignn_gmres64_bytes": (C.c_size_t, [_P]),
    "psignn_gmres64_solve_adjoint": (_INT, [_P, _P, _INT, _P, _P, _P, _P, _P, C.c_double, _INT, _INT, _P, _I64, _P,
                                            C.POINTER(GmresAdjointInfo), C.POINTER(C.c_double), C.POINTER(C.c_double), _P]),
    "psignn_gmres64_solve_shifted": (_INT, [_P, _P, _INT, _P, _P, _P, _P, _P, C.c_double, _INT, C.c_double, _INT, _INT, _P, _I64, _P,
                                            C.POINTER(GmresAdjointInfo), C.POINTER(C.c_double), C.POINTER(C.c_double), _P]),
    "psignn_gmres64_create_aug": (_INT, [C.POINTER(_P), _P, _INT, _INT]),
    "psignn_gmres64_solve_adjoint_opts": (_INT, [_P, _P, _INT, _P, _P, _P, _P, _P, C.c_double, _INT, _INT, C.POINTER(Gmres64Opts), _P, _I64,
                                                 _P, C.POINTER(Gmres64Info), C.POINTER(C.c_double), C.POINTER(C.c_double), _P]),
    "psignn_gmres64_solve_shifted_opts": (_INT, [_P, _P, _INT, _P, _P, _P, _P, _P, C.c_double, _INT, C.c_double, _INT, _INT,
                                                 C.POINTER(Gmres64Opts), _P, _I64, _P, C.POINTER(Gmres64Info), C.POINTER(C.c_double),
                                                 C.POINTER(C.c_double), _P]),
    "psignn_newton64_policy": (C.c_double, [C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.POINTER(_INT)]),
    "psignn_newton64_create": (_INT, [C.POINTER(_P), _P, _INT]),
    "psignn_newton64_destroy": (None, [_P]),
    "psignn_newton64_bytes": (C.c_size_t, [_P]),
    "psignn_newton64_solve": (_INT, [_P, _P, _INT, _P, _P, _P, _P, C.POINTER(Newton64Opts), _P, _I64, _P, C.POINTER(Newton64Info),
                                     C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                     C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P]),
    "psignn_newton64_create_aug": (_INT, [C.POINTER(_P), _P, _INT, _INT]),
    "psignn_newton64_solve_opts": (_INT, [_P, _P, _INT, _P, _P, _P, _P, C.POINTER(Newton64Opts), C.POINTER(Gmres64Opts), _P, _I64, _P,
                                          C.POINTER(Newton64Info), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                          C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P]),
    "psignn_f64_param_vjp_chunk_rows": (_INT, []),
    "psignn_f64_param_vjp_workspace_doubles": (_I64, [_P, _INT]),
    "psignn_f64_param_vjp": (_INT, [_P, _P, _INT, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "psignn_f64_vjp_backward_workspace_doubles": (_I64, [_P, _INT]),
    "psignn_f64_vjp_backward": (_INT, [_P, _P, _INT, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "psignn_f64_vjp_backward_init": (_INT, [_P, _P, _INT, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "psignn_mlp2_f64_backward_workspace_doubles": (_I64, [_I64, _INT, _INT, _INT]),
    "psignn_mlp2_f64_backward": (_INT, [_P, _P, _I64, _INT, _INT, _INT, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "psignn_residual_f64": (_INT, [_P, _P, _P, _P, _P, _P]),
    "psignn_residual_t_f64": (_INT, [_P, _P, _P, _P, _P]),
    "psignn_mse_f64_chunk": (_INT, []),
    "psignn_mse_f64_workspace_doubles": (_I64, [_I64]),
    "psignn_mse_f64": (_INT, [_P, _P, _I64, C.c_double, _P, _P, _P, _I64, _P]),
    "psignn_prof_enable": (None, [_INT]),
    "psignn_reload_knobs": (None, []),
    "psignn_prof_tile_stamps": (None, [_P]),
    "psignn_prof_collect": (_INT, []),
    "psignn_prof_get": (_INT, [_INT, C.c_char_p, _INT, C.POINTER(_I64), C.POINTER(C.c_double)]),
    "psignn_prof_get2": (_INT, [_INT, C.c_char_p, _INT, C.POINTER(_I64), C.POINTER(C.c_double), C.POINTER(_I64)]),
    "psignn_prof_launch": (_INT, [_INT, C.c_char_p, _INT, C.POINTER(C.c_double), C.POINTER(_I64)]),
}


def prof_enable(on: bool, width: int = D):
    """Launch records of the library of ``width`` (each library keeps its own)."""
    lib(width).psignn_prof_enable(int(on))


def prof_collect(with_bytes=False, width: int = D):
    """{kernel name: (calls, total_ms)} of everything the library of ``width`` launched since the last collect (HIP events);
    ``with_bytes``: (calls, total_ms, algorithmic bytes as stated at the launch sites)."""
    l = lib(width)
    out = {}
    for i in range(l.psignn_prof_collect()):
        name = C.create_string_buffer(64)
        calls, ms, byts = _I64(0), C.c_double(0.0), _I64(0)
        check(l.psignn_prof_get2(i, name, 64, C.byref(calls), C.byref(ms), C.byref(byts)), "psignn_prof_get2", l)
        out[name.value.decode()] = (int(calls.value), float(ms.value), int(byts.value)) if with_bytes else (int(calls.value), float(ms.value))
    return out

def prof_launch_log(width: int = D):
    """[(kernel name, ms, algorithmic bytes)] of the launches of the last ``prof_collect``, in launch order."""
    l = lib(width)
    out = []
    for i in range(l.psignn_prof_launch(0, None, 0, None, None)):
        name = C.create_string_buffer(64)
        ms, byts = C.c_double(0.0), _I64(0)
        check(l.psignn_prof_launch(i, name, 64, C.byref(ms), C.byref(byts)), "psignn_prof_launch", l)
        out.append((name.value.decode(), float(ms.value), int(byts.value)))
    return out


_libs = {}   # latent width -> loaded library


def _build_once(path=LIB_PATH):
    """A source checkout without the built libraries (the .so files are kept out of git): compile them in place when hipcc is
    there (one make builds every width).  Nothing else is attempted -- without the library every entry point raises."""
    import shutil
    import subprocess
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(os.path.dirname(LIB_PATH), "csrc")
    if not (os.path.exists(hipcc) and os.path.exists(os.path.join(csrc, "Makefile"))):
        return
    import fcntl
    with open(os.path.join(csrc, ".build.lock"), "w") as lock:   # one builder when several ranks start together
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not os.path.exists(path):
            print(f"[psi-gnn_amd] {os.path.basename(path)} missing: building it with {hipcc} (make -C {csrc})", flush=True)
            r = subprocess.run(["make", "-C", csrc, "-j8", f"HIPCC={hipcc}"], stdout=subprocess.PIPE,
                               stderr=subprocess.STDOUT, text=True)
            if r.returncode != 0 or not os.path.exists(path):
                raise NativeError(f"building {path} failed (make exit code {r.returncode}); last lines of its output:\n"
                                  + "\n".join(r.stdout.splitlines()[-25:]))


def _absent(name, width):
    def raise_forward_only(*args, **kwargs):
        raise forward_only_error(width, name)
    return raise_forward_only


def lib(width: int = D):
    """Load the shared library of a latent width (once each; ``lib()`` is the default width's, with every entry point).  A width
    library binds the entry points it exports; any other name of ``SIGNATURES`` raises the "forward inference only" error when
    called.  Raises NativeError for an unsupported width or if the library has not been built."""
    l = _libs.get(width)
    if l is None:
        width = check_width(width)
        path = lib_path(width)
        if not os.path.exists(path):
            _build_once(path)
        if not os.path.exists(path):
            raise NativeError(
                f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                f"or `make -C psi-gnn_amd/csrc`.  There is no CPU fallback for the HIP path.")
        l = C.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            if width != D and not hasattr(l, name):
                setattr(l, name, _absent(name, width))
                continue
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        if l.psignn_latent_dim() != width:
            raise NativeError(f"{path} was built for latent_dim {l.psignn_latent_dim()}, not {width}")
        l.width = width
        _libs[width] = l
    return l


def check(rc: int, what: str = "", l=None):
    """``l``: the library the call went to (each keeps its own last-error text); the default width's when omitted."""
    if rc != 0:
        msg = (l or lib()).psignn_last_error().decode("utf-8", "replace")
        raise NativeError(f"{what} failed (code {rc}): {msg}")


def stream_ptr(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def ptr(t) -> int:
    """Device pointer of a contiguous tensor (or NULL)."""
    if t is None:
        return 0
    if not t.is_contiguous():
        raise NativeError("tensor handed to the HIP path must be contiguous")
    return t.data_ptr()


def require_cuda(t, name="tensor"):
    if not t.is_cuda:
        raise NativeError(f"{name} is on {t.device}: the HIP path needs device tensors and has no CPU fallback")
