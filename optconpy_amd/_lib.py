"""ctypes binding of ``libricadi_hip.so`` (the C-ABI in ``include/ricadi.h``).

The shared library is the product; there is no CPU fallback.  Importing this
module only loads the library; creating a :class:`Context` needs a visible
MI355X and raises ``RuntimeError`` otherwise.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import scipy.sparse as sps

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RICADI_LIB", os.path.join(_HERE, "libricadi_hip.so"))

RICADI_OK = 0
RICADI_ENOCONV = -3
RICADI_STOP_MAX_STEPS, RICADI_STOP_NEWZ, RICADI_STOP_RES = 0, 1, 2      # ricadi_adi_stop_rule (include/ricadi.h)
RICADI_RADI_SHIFTS_CYCLE, RICADI_RADI_SHIFTS_HAMILTONIAN = 0, 1          # ricadi_set_radi_shifts
RICADI_RADI_SHIFTS_HAMILTONIAN_DOMINANT = 2
RICADI_NEWTON_STOP_MAX_STEPS, RICADI_NEWTON_STOP_ABSTOL, RICADI_NEWTON_STOP_RELTOL = 0, 1, 2   # ricadi_newton_stop_rule
MAX_M = 128
MAX_UPD_COLS = 4096                                                     # ricadi_diff_zzt_fnorm_dev: k1 + k0
# ricadi_version() this mirror was written for: the stats arrays' lengths and the meaning of their slots
# are part of the ABI and are not covered by the struct handshake below
ABI_VERSION = 414


class RicadiOpts(C.Structure):
    _fields_ = [("gmres_tol", C.c_double), ("gmres_restart", C.c_int),
                ("gmres_maxit", C.c_int), ("bj_block", C.c_int), ("agg_v", C.c_int),
                ("agg_p", C.c_int), ("coarse_max", C.c_int), ("use_coarse", C.c_int),
                ("max_levels", C.c_int), ("verbose", C.c_int), ("compress_qr", C.c_int),
                ("hierarchy", C.c_int), ("child_smoother", C.c_int), ("child_damping", C.c_double)]


class RicadiAdiParams(C.Structure):
    _fields_ = [("adi_max_steps", C.c_int), ("adi_newZ_reltol", C.c_double),
                ("adi_res_reltol", C.c_double), ("nwtn_max_steps", C.c_int), ("nwtn_upd_reltol", C.c_double),
                ("nwtn_upd_abstol", C.c_double), ("project_w", C.c_int),
                ("verbose", C.c_int), ("compress_cols", C.c_int), ("sweep_width", C.c_int)]


_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_vp = C.c_void_p
_up = C.POINTER(C.c_uint16)

# name -> (restype, argtypes); every symbol declared in include/ricadi.h
SIGNATURES = {
    "ricadi_last_error": (C.c_char_p, []),
    "ricadi_version": (C.c_int, []),
    "ricadi_sizeof_opts": (C.c_int, []),
    "ricadi_sizeof_adi_params": (C.c_int, []),
    "ricadi_struct_signature": (C.c_char_p, []),
    "ricadi_default_opts": (None, [C.POINTER(RicadiOpts)]),
    "ricadi_default_adi_params": (None, [C.POINTER(RicadiAdiParams)]),
    "ricadi_adi_res_history": (C.c_int, [_vp, _dp, C.c_int, C.POINTER(C.c_int)]),
    "ricadi_set_adi_res_history": (C.c_int, [_vp, C.c_int]),
    "ricadi_adi_stop_rule": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "ricadi_adi_res_launches": (C.c_int, [_vp, C.POINTER(C.c_int64)]),
    "ricadi_newton_history": (C.c_int, [_vp, _dp, C.c_int, C.POINTER(C.c_int)]),
    "ricadi_newton_stop_rule": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "ricadi_diff_zzt_fnorm_dev": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _dp, _dp]),
    "ricadi_create": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "ricadi_destroy": (C.c_int, [_vp]),
    "ricadi_set_opts": (C.c_int, [_vp, C.POINTER(RicadiOpts)]),
    "ricadi_stream": (_vp, [_vp]),
    "ricadi_synchronize": (C.c_int, [_vp]),
    "ricadi_set_operator": (C.c_int, [_vp, C.c_int, C.c_int, _ip, _ip, _dp, _ip, _ip, _dp,
                                      _ip, _ip, _dp]),
    "ricadi_clear_cache": (C.c_int, [_vp]),
    "ricadi_set_dims": (C.c_int, [_vp, C.c_int]),
    "ricadi_set_lowrank": (C.c_int, [_vp, _dp, _dp, C.c_int]),
    "ricadi_spmm": (C.c_int, [_vp, C.c_double, C.c_double, _dp, C.c_int, _dp]),
    "ricadi_precond_apply": (C.c_int, [_vp, C.c_double, C.c_double, _dp, C.c_int, _dp]),
    "ricadi_shift_solve": (C.c_int, [_vp, C.c_double, C.c_double, _dp, _dp, C.c_int, _dp,
                                     C.POINTER(C.c_int), _dp]),
    "ricadi_lyap_adi": (C.c_int, [_vp, _dp, C.c_int, _dp, C.c_int, C.POINTER(RicadiAdiParams),
                                  _dp, C.POINTER(C.c_int), _dp]),
    "ricadi_lyap_adi_cplx": (C.c_int, [_vp, _dp, _dp, C.c_int, _dp, C.c_int, C.POINTER(RicadiAdiParams),
                                       _dp, C.POINTER(C.c_int), _dp]),
    "ricadi_adi_pair_blocks_dev": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, _vp, _vp,
                                             C.c_int, C.c_int, _vp, _dp]),
    "ricadi_adi_pair_info": (C.c_int, [_vp, C.POINTER(C.c_int64)]),
    "ricadi_adi_pair_solve_dev": (C.c_int, [_vp, C.c_double, C.c_double, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _dp]),
    "ricadi_ric_newtonadi": (C.c_int, [_vp, _dp, C.c_int, _dp, C.c_int, _dp, C.c_int, _dp,
                                       C.c_int, _dp, C.POINTER(RicadiAdiParams), _dp, C.c_int,
                                       C.POINTER(C.c_int), _dp]),
    "ricadi_compress": (C.c_int, [_vp, _dp, C.c_int, C.c_double, C.c_int, _dp,
                                  C.POINTER(C.c_int), _dp]),
    "ricadi_recompress": (C.c_int, [_vp, _dp, C.c_int, C.c_double, _dp, C.POINTER(C.c_int)]),
    "ricadi_gain": (C.c_int, [_vp, _ip, _ip, _dp, _dp, C.c_int, _dp, C.c_int, _dp]),
    "ricadi_lyap_res_norm": (C.c_int, [_vp, _dp, C.c_int, _dp, C.c_int, _dp]),
    "ricadi_factor_cols": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "ricadi_factor_get": (C.c_int, [_vp, _dp, C.c_int]),
    "ricadi_factor_set": (C.c_int, [_vp, _dp, C.c_int]),
    "ricadi_factor_get_dev": (C.c_int, [_vp, _vp, C.c_int]),
    "ricadi_ric_newtonadi_dev": (C.c_int, [_vp, _dp, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp,
                                           C.POINTER(RicadiAdiParams), C.POINTER(C.c_int), _dp]),
    "ricadi_ric_radi": (C.c_int, [_vp, _dp, C.c_int, _dp, C.c_int, _dp, C.c_int, _dp, C.c_int, C.c_double, C.c_int,
                                  C.c_int, C.c_int, _dp, C.c_int, C.POINTER(C.c_int), _dp, _dp]),
    "ricadi_ric_radi_dev": (C.c_int, [_vp, _dp, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_double,
                                      C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), _vp, _dp]),
    "ricadi_radi_update_dev": (C.c_int, [_vp, C.c_double, _vp, C.c_int, C.c_int, _vp, C.c_int, _vp, _vp, C.c_int,
                                         C.c_int, _vp, _vp]),
    "ricadi_set_radi_sweep_width": (C.c_int, [_vp, C.c_int]),
    "ricadi_radi_sweep_info": (C.c_int, [_vp, _ip]),
    "ricadi_set_radi_sweep_shifts": (C.c_int, [_vp, C.c_int]),
    "ricadi_radi_sweep_widths": (C.c_int, [_vp, _ip, C.c_int, C.POINTER(C.c_int)]),
    "ricadi_radi_reduce_group_dev": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp]),
    "ricadi_radi_sweep_combine_dev": (C.c_int, [_vp, C.c_int, _vp, C.c_int64, C.c_int, C.c_int, _vp, _vp, C.c_int,
                                                C.c_int, _vp, _vp, C.c_int, C.c_int]),
    "ricadi_set_radi_shifts": (C.c_int, [_vp, C.c_int]),
    "ricadi_set_radi_shift_mode": (C.c_int, [_vp, C.c_int]),
    "ricadi_radi_shift_history": (C.c_int, [_vp, _dp, C.c_int, C.POINTER(C.c_int)]),
    "ricadi_radi_shift_fallbacks": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "ricadi_radi_reduce_dev": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp]),
    "ricadi_radi_reduce_wide_dev": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp]),
    "ricadi_probe_cache_entries": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "ricadi_probe_radi_refuse": (C.c_int, [_vp, _ip, C.c_int]),
    "ricadi_probe_radi_counters": (C.c_int, [_vp, _ip]),
    "ricadi_probe_radi_kept": (C.c_int, [_vp, _ip, C.c_int, C.POINTER(C.c_int)]),
    "ricadi_spmm_dev": (C.c_int, [_vp, C.c_double, C.c_double, _vp, C.c_int, _vp]),
    "ricadi_shift_solve_dev": (C.c_int, [_vp, C.c_double, C.c_double, _vp, C.c_int, _vp,
                                         C.POINTER(C.c_int), _dp]),
    "ricadi_shift_solve_batch_dev": (C.c_int, [_vp, C.c_int, _dp, _dp, _vp, C.c_int64, C.c_int, _vp,
                                               C.POINTER(C.c_int), _dp]),
    "ricadi_time_spmm_batch_dev": (C.c_int, [_vp, C.c_int, _dp, _dp, _vp, C.c_int, _vp, C.c_int,
                                             C.POINTER(C.c_double)]),
    "ricadi_sweep_recombine_dev": (C.c_int, [_vp, C.c_int, _vp, C.c_int, _dp, _dp, _vp, _vp,
                                             C.POINTER(C.c_double)]),
    "ricadi_sweep_recombine_slots_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_int, _dp, _dp, _vp, _vp,
                                                   C.POINTER(C.c_double), _dp]),
    "ricadi_apply_e_dev": (C.c_int, [_vp, C.c_double, _vp, C.c_int, _vp]),
    "ricadi_lincomb_dev": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int64, _dp, _vp]),
    "ricadi_gain_dev": (C.c_int, [_vp, C.c_double, _vp, C.c_int, C.c_int, _vp, C.c_int, _vp]),
    "ricadi_panel_norms_dev": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _dp, _dp]),
    "ricadi_time_spmm_dev": (C.c_int, [_vp, C.c_double, C.c_double, _vp, C.c_int, _vp, C.c_int,
                                       _dp]),
    "ricadi_time_kernel_dev": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int, C.c_int,
                                         C.POINTER(C.c_double)]),
    "ricadi_arnoldi_probe_begin_dev": (C.c_int, [_vp, C.c_int, _dp, _dp, C.c_int, _vp, _vp]),
    "ricadi_arnoldi_probe_step_dev": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.POINTER(C.c_int)]),
    "ricadi_arnoldi_probe_close_dev": (C.c_int, [_vp, C.POINTER(C.c_int), C.c_int, _vp, _vp]),
    "ricadi_arnoldi_probe_read_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_int64, C.POINTER(C.c_int64)]),
    "ricadi_qr": (C.c_int, [_vp, _dp, C.c_int, _dp, _dp]),
    "ricadi_project_pencil": (C.c_int, [_vp, _dp, C.c_int, _dp, _dp]),
    "ricadi_project_pencil_dev": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp]),
    "ricadi_cross_gram_dev": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp]),
    "ricadi_project_pencil_twosided_dev": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp]),
    "ricadi_lqg_balance_dev": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_double,
                                         C.c_int, C.POINTER(C.c_int), _dp, _vp, _vp, _dp, _dp, _dp, _dp]),
    "ricadi_host_lqg_balance": (C.c_int, [C.c_int, C.c_int, _dp, C.c_double, C.c_int, C.POINTER(C.c_int), _dp, _dp,
                                          _dp]),
    "ricadi_setup_info": (C.c_int, [_vp, C.POINTER(C.c_int), C.c_int]),
    "ricadi_time_qr_dev": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "ricadi_time_gram_dev": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _dp]),
    "ricadi_set_recycle": (C.c_int, [_vp, C.c_int]),
    "ricadi_recycle_guess_dev": (C.c_int, [_vp, C.c_int, _dp, _dp, _vp, C.c_int, _vp, C.POINTER(C.c_int)]),
    "ricadi_solve_trace": (C.c_int, [_vp, C.POINTER(C.c_int64), C.c_int]),
    "ricadi_set_exchange": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, C.c_int64]),
    "ricadi_rccl_unique_id": (C.c_int, [_vp, C.c_int]),
    "ricadi_set_exchange_rccl": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, C.c_int64]),
    "ricadi_exchange_count": (C.c_int, [_vp, C.POINTER(C.c_int64)]),
    "ricadi_dense_inverse_batch": (C.c_int, [_vp, C.c_int, C.c_int, _dp, C.POINTER(C.c_int)]),
    "ricadi_precond_apply_batch_dev": (C.c_int, [_vp, C.c_int, _dp, _dp, _vp, C.c_int64, C.c_int, _ip, C.c_int,
                                                 _vp, C.POINTER(C.c_int)]),
    "ricadi_precond_structure": (C.c_int, [_vp, C.c_int, _ip, _ip, _ip, _ip, _ip, _ip, _ip, _ip, _dp]),
    "ricadi_op_apply_batch_dev": (C.c_int, [_vp, C.c_int, _dp, _dp, _vp, C.c_int64, C.c_int, _ip, C.c_int, C.c_int,
                                            C.c_double, _vp, C.c_int64, C.c_double, _vp, C.c_int64,
                                            C.POINTER(C.c_int)]),
    "ricadi_shift_solve_cplx_batch_dev": (C.c_int, [_vp, C.c_int, _dp, _dp, _dp, _vp, C.c_int64, C.c_int, _vp,
                                                    C.POINTER(C.c_int), _dp]),
    "ricadi_op_apply_cplx_batch_dev": (C.c_int, [_vp, C.c_int, _dp, _dp, _dp, _vp, C.c_int64, C.c_int, _ip, C.c_int,
                                                 _vp, C.c_int64, C.POINTER(C.c_int)]),
    "ricadi_cplx_orth_dev": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int64, C.c_int64, _vp, _vp]),
    "ricadi_host_cplx_proxy": (C.c_int, [C.c_double, C.c_double, C.POINTER(C.c_double)]),
    "ricadi_cplx_probe_begin_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _dp]),
    "ricadi_cplx_probe_step_dev": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.POINTER(C.c_int)]),
    "ricadi_cplx_probe_close_dev": (C.c_int, [_vp, C.POINTER(C.c_int), C.c_int, _vp, _vp]),
    "ricadi_cplx_probe_read_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_int64, C.POINTER(C.c_int64)]),
    "ricadi_host_saddle_tiles": (C.c_int, [C.c_int, C.c_int, _ip, _ip, _dp, _ip, _ip, _dp, _ip, _ip, _dp,
                                           C.POINTER(RicadiOpts), _ip, _ip, _ip, _ip, _up, _up, _dp, _dp, _ip, _ip,
                                           _ip, _dp]),
    "ricadi_host_deal": (C.c_int, [_dp, C.c_int, C.c_int, _ip]),
    "ricadi_host_sa_criterion": (C.c_int, [C.c_int, _ip, _ip, _dp, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                           C.POINTER(C.c_int)]),
    "ricadi_host_plan_levels": (C.c_int, [C.c_int, C.c_int, _ip, _ip, _dp, _ip, _ip, _dp, _ip, _ip, _dp,
                                          C.POINTER(RicadiOpts), _ip]),
    "ricadi_host_plan_hierarchy": (C.c_int, [C.c_int, C.c_int, _ip, _ip, _dp, _ip, _ip, _dp, _ip, _ip, _dp,
                                             C.POINTER(RicadiOpts), _ip, _ip, _ip]),
    "ricadi_host_aggregate": (C.c_int, [C.c_int, _ip, _ip, C.c_int, _ip]),
    "ricadi_host_vanka_patches": (C.c_int, [C.c_int, C.c_int, _ip, _ip, _dp, _ip, _ip, _ip]),
    "ricadi_precond_vanka": (C.c_int, [_vp, C.c_int, _ip, _ip, _ip]),
    "ricadi_host_cauchy": (C.c_int, [_dp, C.c_int, _dp, _dp]),
    "ricadi_host_adi_window_width": (C.c_int, [_dp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "ricadi_host_radi_shift": (C.c_int, [C.c_int, C.c_int, C.c_int, _dp, C.POINTER(C.c_double),
                                         C.POINTER(C.c_double)]),
    "ricadi_host_radi_shift_eigs": (C.c_int, [C.c_int, C.c_int, C.c_int, _dp, C.POINTER(C.c_double),
                                              C.POINTER(C.c_double), _dp, _dp]),
    "ricadi_host_radi_next_shift": (C.c_int, [C.c_int, C.c_int, _dp, _dp, C.POINTER(C.c_double),
                                              C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "ricadi_host_radi_next_shift_dominant": (C.c_int, [C.c_int, C.c_int, _dp, _dp, C.POINTER(C.c_double),
                                                       C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "ricadi_host_radi_sweep": (C.c_int, [C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, C.c_double, C.c_double, C.c_int,
                                         C.POINTER(C.c_int), _dp, _dp]),
    "ricadi_host_radi_sweep_width": (C.c_int, [_dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                               C.POINTER(C.c_int)]),
    "ricadi_host_radi_sweep_shifts": (C.c_int, [C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_int, _dp, _dp,
                                                C.POINTER(C.c_int), C.POINTER(C.c_int)]),
}

EXCHANGE_FN = C.CFUNCTYPE(C.c_int, _vp, _vp, _vp, C.c_int64)

_lib = None


def load():
    """Load the shared library (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libricadi_hip.so is missing ({0}); build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` -- there is no "
            "CPU fallback for the HIP path".format(LIB_PATH))
    # torch wheels bundle their own ROCm runtime (libamdhip64 / rocblas /
    # rocsolver, same SONAMEs as /opt/rocm).  Two HIP runtimes in one process
    # crash, so torch -- needed anyway for torch.distributed -- is imported
    # first and our NEEDED entries then bind to the already loaded copies.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.ricadi_version() != ABI_VERSION:
        raise RuntimeError("{0}: library ABI version {1}, optconpy_amd/_lib.py was written for {2} -- rebuild "
                           "the library (__graft_entry__.build()) or update the mirror"
                           .format(LIB_PATH, lib.ricadi_version(), ABI_VERSION))
    # struct handshake: the library reads every field of the structs it is handed, so a
    # mirror that is shorter than the library's struct makes it read past our buffer
    # (root cause of the round-1 abort: a rebuilt .so with a new ricadi_adi_params field
    # met a not-yet-updated mirror).  Refuse to run with a mismatched build.
    for what, ours, theirs in (("ricadi_opts", C.sizeof(RicadiOpts), lib.ricadi_sizeof_opts()),
                               ("ricadi_adi_params", C.sizeof(RicadiAdiParams),
                                lib.ricadi_sizeof_adi_params())):
        if ours != theirs:
            raise RuntimeError("{0}: struct {1} is {2} bytes in the library but {3} bytes in "
                               "optconpy_amd/_lib.py -- rebuild the library (__graft_entry__.build())"
                               .format(LIB_PATH, what, theirs, ours))
    ours = ";".join("{0}:{1}".format(nm, "".join("d" if t is C.c_double else "i" for _, t in st._fields_))
                    for nm, st in (("ricadi_opts", RicadiOpts), ("ricadi_adi_params", RicadiAdiParams)))
    theirs = lib.ricadi_struct_signature().decode()
    if ours != theirs:
        raise RuntimeError("{0}: struct layout '{1}' in the library, '{2}' in optconpy_amd/_lib.py "
                           "-- rebuild the library or update the mirror".format(LIB_PATH, theirs, ours))
    _lib = lib
    return lib


def _chk(rc, allow_noconv=False):
    if rc == RICADI_OK or (allow_noconv and rc == RICADI_ENOCONV):
        return rc
    msg = load().ricadi_last_error().decode("utf-8", "replace")
    if rc == -1:
        raise ValueError("ricadi: " + msg)
    raise RuntimeError("ricadi error {0}: {1}".format(rc, msg))


def _d(a):
    return a.ctypes.data_as(_dp)


def _i(a):
    return a.ctypes.data_as(_ip)


def as_panel(a, nrows=None):
    """C-contiguous float64 2-D array (column vectors become n x 1)."""
    if sps.issparse(a):
        a = a.toarray()
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 1:
        a = a.reshape(-1, 1)
    a = np.ascontiguousarray(a)
    if nrows is not None and a.shape[0] != nrows:
        raise ValueError("panel has {0} rows, expected {1}".format(a.shape[0], nrows))
    return a


def as_csr(a):
    """Sorted CSR with int32 indices and float64 values (input csr / csc / dense)."""
    m = sps.csr_matrix(a, dtype=np.float64)
    m.sum_duplicates()
    m.sort_indices()
    if m.nnz >= 2 ** 31:
        raise ValueError("matrix too large for int32 indices")
    return (np.ascontiguousarray(m.indptr, dtype=np.int32),
            np.ascontiguousarray(m.indices, dtype=np.int32),
            np.ascontiguousarray(m.data, dtype=np.float64), m.shape)


def _warn_nonconverged(info):
    """Non-convergence of an inner solve is not an error at the C-ABI (the outer
    loops go on, like the reference's when it hits *_max_steps) -- but say so."""
    if info.get("gmres_nonconverged", 0):
        import warnings
        warnings.warn("ricadi: {0} of {1} shift-solves stopped at gmres_maxit above the tolerance "
                      "(worst relative residual {2:.1e}); the low-rank factor may be inaccurate"
                      .format(info["gmres_nonconverged"], info["shift_solves"],
                              info["gmres_worst_relres"]), RuntimeWarning, stacklevel=3)


def default_opts(**kw):
    o = RicadiOpts()
    load().ricadi_default_opts(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise KeyError("unknown ricadi option " + k)
        setattr(o, k, v)
    return o


def adi_params(d=None, project_w=True):
    """Translate the reference's ``nwtn_adi_dict`` (optcont_main.py:122-131).

    Unknown keys are ignored, missing ones take the reference defaults.
    """
    p = RicadiAdiParams()
    load().ricadi_default_adi_params(C.byref(p))
    d = {} if d is None else d
    for k in ("adi_max_steps", "nwtn_max_steps"):
        if k in d:
            setattr(p, k, int(d[k]))
    for k in ("adi_newZ_reltol", "nwtn_upd_reltol", "nwtn_upd_abstol", "adi_res_reltol"):
        if k in d:
            setattr(p, k, float(d[k]))
    p.verbose = 1 if d.get("verbose", False) else 0
    p.project_w = 1 if d.get("project_w", project_w) else 0
    p.compress_cols = int(d.get("compress_cols", 0))
    p.sweep_width = int(d.get("sweep_width", 1))
    return p


class Context:
    """One GPU, one stream, one saddle-point operator."""

    def __init__(self, device=0, **opts):
        self._lib = load()
        self._h = _vp()
        _chk(self._lib.ricadi_create(int(device), C.byref(self._h)))
        self.nv = self.np_ = self.n = 0
        self._lowrank = None
        self.diag_ratio = None
        if opts:
            self.set_opts(**opts)

    # -- lifetime ---------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.ricadi_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def stream(self):
        return self._lib.ricadi_stream(self._h)

    def synchronize(self):
        _chk(self._lib.ricadi_synchronize(self._h))

    def set_opts(self, **kw):
        o = default_opts(**kw)
        self._opts = o
        _chk(self._lib.ricadi_set_opts(self._h, C.byref(o)))

    # -- operator ---------------------------------------------------------
    def set_operator(self, calA, calE, J=None):
        """``calA``, ``calE`` NV x NV, ``J`` NP x NV (or None), any scipy format."""
        self._zdev = None
        arp, aci, av, ash = as_csr(calA)
        erp, eci, ev, esh = as_csr(calE)
        nv = ash[0]
        if ash != (nv, nv) or esh != (nv, nv):
            raise ValueError("calA / calE must be square and of equal size")
        if J is not None and J.shape[0] > 0:
            jrp, jci, jv, jsh = as_csr(J)
            if jsh[1] != nv:
                raise ValueError("J has the wrong number of columns")
            np_ = jsh[0]
            _chk(self._lib.ricadi_set_operator(self._h, nv, np_, _i(arp), _i(aci), _d(av),
                                               _i(erp), _i(eci), _d(ev), _i(jrp), _i(jci),
                                               _d(jv)))
        else:
            np_ = 0
            _chk(self._lib.ricadi_set_operator(self._h, nv, 0, _i(arp), _i(aci), _d(av),
                                               _i(erp), _i(eci), _d(ev), None, None, None))
        self.nv, self.np_ = nv, np_
        self.n = nv + np_
        self._lowrank = None
        # |diag cal A / diag cal E| over the velocity dofs where both are nonzero: the initial shift estimate of
        # adi_shifts.auto_shifts
        da, de = sps.csr_matrix(calA).diagonal(), sps.csr_matrix(calE).diagonal()
        ok = (da != 0) & (de != 0)
        self.diag_ratio = np.abs(da[ok] / de[ok])

    def clear_cache(self):
        _chk(self._lib.ricadi_clear_cache(self._h))

    def set_dims(self, nv):
        """Dimension-only context: enough for compress() and gain(MT=...)."""
        self._zdev = None
        _chk(self._lib.ricadi_set_dims(self._h, int(nv)))
        self.nv, self.np_, self.n = int(nv), 0, int(nv)

    def set_lowrank(self, U=None, V=None):
        """Operator becomes ``beta*A + alpha*E - U V^T`` (both NV x q)."""
        if U is None or V is None:
            _chk(self._lib.ricadi_set_lowrank(self._h, None, None, 0))
            self._lowrank = None
            return
        U = as_panel(U, self.nv)
        V = as_panel(V, self.nv)
        if U.shape != V.shape:
            raise ValueError("U and V must have the same shape")
        _chk(self._lib.ricadi_set_lowrank(self._h, _d(U), _d(V), U.shape[1]))
        self._lowrank = (U, V)

    def set_recycle(self, depth):
        """Depth of the recycling ring for DIRECT solve calls (the ADI drivers use their own, 3)."""
        _chk(self._lib.ricadi_set_recycle(self._h, int(depth)))
        self.recycle_depth = int(depth)

    def set_exchange(self, group=None, panel_cols=MAX_M, per_rank=2, transport=None):
        """Shard the ADI sweeps of this context over the ranks of a ``torch.distributed`` process group
        (SURVEY.md 8e): ONE all-gather of the solution panels per sweep, ``per_rank`` panels of
        ``n x panel_cols`` per rank.  ``transport``:

        * ``"rccl"`` (default for groups of the nccl backend): the library joins an RCCL communicator of its
          own -- rank 0's ``ncclGetUniqueId`` bytes go round through the group -- and enqueues
          ``ncclAllGather`` on its stream between the solves and the recombination (``ricadi_set_exchange_rccl``):
          no host synchronisation, no Python in the sweep;
        * ``"callback"`` (gloo groups: CPU tests, several ranks on one GPU): the library calls back for
          ``all_gather_into_tensor`` on two device buffers allocated here.

        ``group=False`` removes the exchange."""
        import torch
        import torch.distributed as dist
        if group is False or not (dist.is_available() and dist.is_initialized()):
            _chk(self._lib.ricadi_set_exchange(self._h, 0, 1, None, None, None, None, 0))
            self._xchg = None
            return
        world, rank = dist.get_world_size(group), dist.get_rank(group)
        if transport is None:
            transport = "rccl" if dist.get_backend(group) == "nccl" else "callback"
        if world == 1 and transport != "rccl":
            _chk(self._lib.ricadi_set_exchange(self._h, 0, 1, None, None, None, None, 0))
            self._xchg = None
            return
        count = int(per_rank) * self.n * int(panel_cols) + 512        # + 4096 bytes of control messages
        if transport == "rccl":
            cur = getattr(self, "_xchg", None)
            if cur is not None and cur[0] == "rccl" and cur[3] is group:
                # same communicator, larger buffers (wider panels)
                _chk(self._lib.ricadi_set_exchange_rccl(self._h, rank, world, None, None, count * 8))
                self._xchg = ("rccl", None, None, group, count)
                return
            ident = [None]
            if rank == 0:
                buf = C.create_string_buffer(128)
                _chk(self._lib.ricadi_rccl_unique_id(buf, 128))
                ident[0] = buf.raw
            if world > 1:
                dist.broadcast_object_list(ident, src=dist.get_global_rank(group, 0) if group is not None else 0,
                                           group=group)
            torch.cuda.synchronize()
            rc = self._lib.ricadi_set_exchange_rccl(self._h, rank, world, ident[0], None, count * 8)
            ok = torch.tensor([1 if rc == 0 else 0], dtype=torch.int32, device="cuda")
            if world > 1:
                dist.all_reduce(ok, op=dist.ReduceOp.MIN, group=group)       # all ranks take the same transport
            if int(ok.item()) == 1:
                self._xchg = ("rccl", None, None, group, count)
                return
            import warnings
            warnings.warn("ricadi: the library's own RCCL communicator could not be set up ({0}); the all-gather of the "
                          "sharded sweeps goes through torch.distributed instead".format(
                              self._lib.ricadi_last_error().decode() if rc != 0 else "another rank failed"),
                          RuntimeWarning)
            _chk(self._lib.ricadi_set_exchange(self._h, 0, 1, None, None, None, None, 0))
            if world == 1:
                self._xchg = None
                return
        dev = torch.device("cuda", torch.cuda.current_device())
        send = torch.zeros(count, dtype=torch.float64, device=dev)
        recv = torch.zeros(count * world, dtype=torch.float64, device=dev)

        def gather(user, sptr, rptr, nbytes):
            try:
                k = int(nbytes) // 8
                so = (int(sptr) - send.data_ptr()) // 8           # the library also calls with pointers INTO the
                ro = (int(rptr) - recv.data_ptr()) // 8           # buffers (control messages in their tails)
                dist.all_gather_into_tensor(recv[ro:ro + k * world], send[so:so + k], group=group)
                torch.cuda.current_stream().synchronize()
                return 0
            except Exception as e:                        # never unwind through the C frames
                import sys
                print("ricadi exchange callback: {0!r}".format(e), file=sys.stderr, flush=True)
                return 1

        cb = EXCHANGE_FN(gather)
        torch.cuda.synchronize()
        _chk(self._lib.ricadi_set_exchange(self._h, rank, world, C.cast(cb, _vp), None, send.data_ptr(),
                                           recv.data_ptr(), count * 8))
        self._xchg = (cb, send, recv, group, count)          # keep the callback and the buffers alive

    def exchange_count(self):
        """Collectives this context has issued so far (one per sharded ADI sweep + control messages)."""
        k = C.c_int64(0)
        _chk(self._lib.ricadi_exchange_count(self._h, C.byref(k)))
        return int(k.value)

    # -- kernels ----------------------------------------------------------
    def _need_op(self):
        if not self.n:
            raise RuntimeError("ricadi: no operator set on this context")

    def spmm(self, alpha, beta, X):
        self._need_op()
        X = as_panel(X, self.n)
        Y = np.empty_like(X)
        _chk(self._lib.ricadi_spmm(self._h, alpha, beta, _d(X), X.shape[1], _d(Y)))
        return Y

    def precond_apply(self, alpha, beta, R):
        self._need_op()
        R = as_panel(R, self.n)
        Z = np.empty_like(R)
        _chk(self._lib.ricadi_precond_apply(self._h, alpha, beta, _d(R), R.shape[1], _d(Z)))
        return Z

    def shift_solve(self, alpha, beta, R, Rp=None, strict=True):
        """Solve ``S(alpha,beta) [V;L] = [R;Rp]``; wide panels go in chunks."""
        self._need_op()
        R = as_panel(R, self.nv)
        m = R.shape[1]
        Rp = None if Rp is None else as_panel(Rp, self.np_)
        X = np.empty((self.n, m))
        iters, relres = 0, np.zeros(m)
        for c0 in range(0, m, MAX_M):
            c1 = min(m, c0 + MAX_M)
            Rc = np.ascontiguousarray(R[:, c0:c1])
            Rpc = None if Rp is None else np.ascontiguousarray(Rp[:, c0:c1])
            Xc = np.empty((self.n, c1 - c0))
            it = C.c_int(0)
            rr = np.zeros(c1 - c0)
            rc = self._lib.ricadi_shift_solve(self._h, alpha, beta, _d(Rc),
                                              None if Rpc is None else _d(Rpc), c1 - c0,
                                              _d(Xc), C.byref(it), _d(rr))
            _chk(rc, allow_noconv=not strict)
            X[:, c0:c1] = Xc
            iters += it.value
            relres[c0:c1] = rr
        return X, iters, relres

    # -- solvers ----------------------------------------------------------
    STOP_RULES = ("max_steps", "newZ", "res")

    def set_adi_res_history(self, on):
        """Record the relative Lyapunov residual after every ADI step also while ``adi_res_reltol`` is 0."""
        _chk(self._lib.ricadi_set_adi_res_history(self._h, 1 if on else 0))

    def adi_res_history(self):
        """``ricadi_adi_res_history``: the relative residual after every step of the last Lyapunov solve
        (empty unless ``adi_res_reltol > 0`` or :meth:`set_adi_res_history` asked for it)."""
        n = C.c_int(0)
        _chk(self._lib.ricadi_adi_res_history(self._h, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1))
        _chk(self._lib.ricadi_adi_res_history(self._h, _d(out), n.value, C.byref(n)))
        return out[:n.value].copy()

    def adi_res_launches(self):
        """Kernel launches the residual rule has added on this context so far (0 while it is off)."""
        n = C.c_int64(0)
        _chk(self._lib.ricadi_adi_res_launches(self._h, C.byref(n)))
        return int(n.value)

    def adi_stopped_by(self):
        """``ricadi_adi_stop_rule`` of the last Lyapunov solve: ``'newZ'``, ``'res'`` or ``'max_steps'``."""
        r = C.c_int(0)
        _chk(self._lib.ricadi_adi_stop_rule(self._h, C.byref(r)))
        return self.STOP_RULES[r.value]

    NEWTON_STOP_RULES = ("max_steps", "abstol", "reltol")

    def newton_history(self, cap=None):
        """``ricadi_newton_history``: one row ``[upd_abs, upd_rel, ADI steps, raw columns, columns kept,
        ||Z_new Z_new^T||_F]`` per Newton step of the last Newton call.  ``cap``: copy at most that many rows;
        returns ``(rows, steps of the call)`` then."""
        n = C.c_int(0)
        _chk(self._lib.ricadi_newton_history(self._h, None, 0, C.byref(n)))
        rows = n.value if cap is None else int(cap)
        out = np.full((max(rows, 1), 6), np.nan)
        _chk(self._lib.ricadi_newton_history(self._h, _d(out), rows, C.byref(n)))
        hist = out[:min(rows, n.value)].copy()
        return hist if cap is None else (hist, n.value)

    def newton_stopped_by(self):
        """``ricadi_newton_stop_rule`` of the last Newton call: ``'abstol'``, ``'reltol'`` or ``'max_steps'``
        (``'abstol'`` where both tolerances were met at one step)."""
        r = C.c_int(0)
        _chk(self._lib.ricadi_newton_stop_rule(self._h, C.byref(r)))
        return self.NEWTON_STOP_RULES[r.value]

    def diff_zzt_fnorm_dev(self, z1_ptr, k1, z0_ptr, k0, want=(True, True)):
        """``ricadi_diff_zzt_fnorm_dev``: ``(||Z1 Z1^T - Z0 Z0^T||_F, ||Z1 Z1^T||_F)`` of two device panels (row-major,
        leading dimension = width; ``z0_ptr`` None with ``k0 = 0``), as the Newton loop forms them.  ``want``: which of
        the two outputs to pass (the other pointer is NULL and its value comes back as NaN)."""
        upd, x1 = C.c_double(np.nan), C.c_double(np.nan)
        _chk(self._lib.ricadi_diff_zzt_fnorm_dev(self._h, z1_ptr, int(k1), z0_ptr, int(k0),
                                                 C.byref(upd) if want[0] else None, C.byref(x1) if want[1] else None))
        return upd.value, x1.value

    def lyap_adi(self, shifts, W, prm, fetch=True):
        """``ricadi_lyap_adi``; a list with a complex entry -- one number ``p`` with ``Re p < 0`` that stands for the
        pair ``(p, conj p)``, DESIGN.md 3g -- goes through ``ricadi_lyap_adi_cplx`` and adds ``info['pair_info']``
        (:meth:`adi_pair_info`)."""
        W = as_panel(W, self.nv)
        m = W.shape[1]
        shc = np.asarray(shifts)
        pairs = np.iscomplexobj(shc) and bool(np.any(shc.imag != 0.0))
        sh = np.ascontiguousarray(shc.real, dtype=np.float64)
        cap = prm.adi_max_steps * m
        Z = np.empty((self.nv, cap)) if fetch else None
        cc = C.c_int(0)
        stats = np.zeros(8)
        self._zdev = None
        if pairs:
            shi = np.ascontiguousarray(shc.imag, dtype=np.float64)
            _chk(self._lib.ricadi_lyap_adi_cplx(self._h, _d(sh), _d(shi), sh.size, _d(W), m, C.byref(prm),
                                                None if Z is None else _d(Z), C.byref(cc), _d(stats)))
        else:
            _chk(self._lib.ricadi_lyap_adi(self._h, _d(sh), sh.size, _d(W), m, C.byref(prm),
                                           None if Z is None else _d(Z), C.byref(cc), _d(stats)))
        c = cc.value
        if fetch:
            Z = Z.ravel()[:self.nv * c].reshape(self.nv, c)
        info = dict(adi_steps=int(stats[0]), adi_rel_newZ=stats[1], gmres_iters=int(stats[2]),
                    shift_solves=int(stats[3]), res_fro=stats[4], cols=c,
                    gmres_nonconverged=int(stats[5]), gmres_worst_relres=stats[6],
                    storage_escalations=int(stats[7]), adi_stopped_by=self.adi_stopped_by())
        if pairs:
            info["pair_info"] = self.adi_pair_info()
        _warn_nonconverged(info)
        return Z, info

    def lyap_adi_cplx(self, shifts_re, shifts_im, W, prm):
        """``ricadi_lyap_adi_cplx`` as it is, for tests: returns ``(Z, stats[8], columns)``."""
        W = as_panel(W, self.nv)
        m = W.shape[1]
        sr = np.ascontiguousarray(shifts_re, dtype=np.float64)
        si = np.ascontiguousarray(shifts_im, dtype=np.float64)
        Z = np.empty((self.nv, prm.adi_max_steps * m))
        cc = C.c_int(0)
        stats = np.zeros(8)
        self._zdev = None
        _chk(self._lib.ricadi_lyap_adi_cplx(self._h, _d(sr), _d(si), sr.size, _d(W), m, C.byref(prm), _d(Z),
                                            C.byref(cc), _d(stats)))
        return Z.ravel()[:self.nv * cc.value].reshape(self.nv, cc.value), stats, cc.value

    def adi_pair_info(self):
        """``ricadi_adi_pair_info`` of the last ``ricadi_lyap_adi_cplx`` call: ``[pairs solved, lockstep iterations of
        the complex GMRES, Woodbury refinement passes, complex solves that missed the tolerance]``."""
        out = (C.c_int64 * 4)()
        _chk(self._lib.ricadi_adi_pair_info(self._h, out))
        return [int(v) for v in out]

    def adi_pair_blocks_dev(self, ng, mc, m, p, x_ptr, z_ptr, ldz, zc, v1_ptr):
        """``ricadi_adi_pair_blocks_dev``: the blocks kernel of the pair step at ``p`` on device panels; returns the two
        squared block norms."""
        out = np.zeros(2)
        p = complex(p)
        _chk(self._lib.ricadi_adi_pair_blocks_dev(self._h, int(ng), int(mc), int(m), p.real, p.imag, x_ptr, z_ptr,
                                                  int(ldz), int(zc), v1_ptr, _d(out)))
        return out

    PAIR_SOLVE_RHS, PAIR_SOLVE_RAW, PAIR_SOLVE_X, PAIR_SOLVE_PACK_ONLY = 1, 2, 4, 8
    PAIR_SOLVE_REPORT = ("ng", "mc", "iters", "refined", "worst_before", "worst_after", "converged", "min_pivot_rel")

    def adi_pair_solve_dev(self, p, w_ptr, m, what_mask=0, raw_ptr=None, x_ptr=None, rhs_ptr=None):
        """``ricadi_adi_pair_solve_dev``: the complex solve of one pair entry at ``p`` for the device panel ``W``
        (``nv x m``), as the driver runs it, with the outputs ``what_mask`` asks for (``PAIR_SOLVE_*``) copied to the
        device buffers.  Returns the report as a dict (``PAIR_SOLVE_REPORT``); when the call fails the report filled so
        far is ``self.pair_solve_report`` (``None`` after a refusal, which writes nothing)."""
        rep = np.full(8, -1.0)
        p = complex(p)
        self.pair_solve_report = None
        rc = self._lib.ricadi_adi_pair_solve_dev(self._h, p.real, p.imag, w_ptr, int(m), int(what_mask), raw_ptr, x_ptr,
                                                 rhs_ptr, _d(rep))
        out = dict(zip(self.PAIR_SOLVE_REPORT, rep.tolist()))
        for k in ("ng", "mc", "iters"):
            out[k] = int(out[k])
        for k in ("refined", "converged"):
            out[k] = bool(out[k])
        if rc != 0 and rep[0] >= 0:
            self.pair_solve_report = out
        _chk(rc)
        return out

    def ric_newtonadi(self, shifts, B, W, prm, Z0=None, oldB=None, fetch=True, upd_hist=False):
        """``upd_hist=True`` adds ``info['upd_hist']`` (:meth:`newton_history` of this call) and
        ``info['nwtn_stopped_by']``.  They come on request only: without them every value of ``info`` is a number or a
        string, and callers convert the dict wholesale on that footing (``tests/context_battery.py`` does)."""
        B = as_panel(B, self.nv)
        W = as_panel(W, self.nv)
        sh = np.ascontiguousarray(shifts, dtype=np.float64)
        nb, mw = B.shape[1], W.shape[1]
        Z0 = None if Z0 is None else as_panel(Z0, self.nv)
        oldB = None if oldB is None else as_panel(oldB, self.nv)
        cap = prm.adi_max_steps * (mw + nb)
        Z = np.empty((self.nv, cap)) if fetch else None
        cc = C.c_int(0)
        stats = np.zeros(12)
        self._zdev = None
        _chk(self._lib.ricadi_ric_newtonadi(
            self._h, _d(sh), sh.size, _d(B), nb, _d(W), mw,
            None if Z0 is None else _d(Z0), 0 if Z0 is None else Z0.shape[1],
            None if oldB is None else _d(oldB), C.byref(prm),
            None if Z is None else _d(Z), cap, C.byref(cc), _d(stats)))
        c = cc.value
        if fetch:
            Z = Z.ravel()[:self.nv * c].reshape(self.nv, c)
            # The factor also stays on the device.  The returned array is made read-only, so that a later
            # gain(B, Z=<this very array>) may use the device copy instead of uploading it again
            # (get_mTzzTtb right after the Newton iteration: optcont_main.py:488-506).
            Z.flags.writeable = False
            self._zdev = Z
        info = dict(nwtn_steps=int(stats[0]), upd_abs=stats[1], upd_rel=stats[2],
                    adi_steps=int(stats[3]), gmres_iters=int(stats[4]),
                    shift_solves=int(stats[5]), cols=c,
                    gmres_nonconverged=int(stats[6]), gmres_worst_relres=stats[7],
                    lyap_res_fro=stats[8], lyap_rhs_fro=stats[9], storage_escalations=int(stats[10]),
                    adi_sweeps=int(stats[11]), adi_stopped_by=self.adi_stopped_by())
        if upd_hist:
            info.update(upd_hist=self.newton_history(), nwtn_stopped_by=self.newton_stopped_by())
        _warn_nonconverged(info)
        return Z, info

    def factor_get_dev(self, z_ptr, c):
        """Copy the context's resident factor (NV x c, packed) into a device buffer."""
        _chk(self._lib.ricadi_factor_get_dev(self._h, z_ptr, int(c)))

    def ric_newtonadi_dev(self, shifts, B_t, W_t, prm, Z0_t=None, old_t=None, upd_hist=False):
        """``ricadi_ric_newtonadi_dev``: every panel is a torch CUDA tensor (float64, contiguous, NV rows);
        the new iterate comes back as a fresh NV x c CUDA tensor.  No PCIe traffic.  ``upd_hist``: as
        :meth:`ric_newtonadi`."""
        import torch
        sh = np.ascontiguousarray(shifts, dtype=np.float64)
        for t in (B_t, W_t, Z0_t, old_t):
            if t is not None and not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()
                                      and t.dim() == 2 and t.shape[0] == self.nv):
                raise ValueError("device panels must be contiguous float64 CUDA tensors with NV rows")
        cc = C.c_int(0)
        stats = np.zeros(12)
        self._zdev = None
        torch.cuda.current_stream().synchronize()          # the library runs on its own stream
        _chk(self._lib.ricadi_ric_newtonadi_dev(
            self._h, _d(sh), sh.size, B_t.data_ptr(), B_t.shape[1], W_t.data_ptr(), W_t.shape[1],
            None if Z0_t is None else Z0_t.data_ptr(), 0 if Z0_t is None else Z0_t.shape[1],
            None if old_t is None else old_t.data_ptr(), C.byref(prm), C.byref(cc), _d(stats)))
        c = cc.value
        Zt = torch.empty((self.nv, c), dtype=torch.float64, device=B_t.device)
        if c > 0:
            _chk(self._lib.ricadi_factor_get_dev(self._h, Zt.data_ptr(), c))
        info = dict(nwtn_steps=int(stats[0]), upd_abs=stats[1], upd_rel=stats[2],
                    adi_steps=int(stats[3]), gmres_iters=int(stats[4]),
                    shift_solves=int(stats[5]), cols=c,
                    gmres_nonconverged=int(stats[6]), gmres_worst_relres=stats[7],
                    lyap_res_fro=stats[8], lyap_rhs_fro=stats[9], storage_escalations=int(stats[10]),
                    adi_sweeps=int(stats[11]), adi_stopped_by=self.adi_stopped_by())
        if upd_hist:
            info.update(upd_hist=self.newton_history(), nwtn_stopped_by=self.newton_stopped_by())
        _warn_nonconverged(info)
        return Zt, info

    @staticmethod
    def _radi_info(stats, c, rule):
        return dict(radi_steps=int(stats[0]), res_rel=stats[1], rhs_fro=stats[2], gmres_iters=int(stats[3]),
                    shift_solves=int(stats[4]), cols=c, gmres_nonconverged=int(stats[5]),
                    gmres_worst_relres=stats[6], storage_escalations=int(stats[7]), stop_rule=rule)

    def ric_radi(self, shifts, B, W, oldB=None, max_steps=200, res_reltol=1e-10, compress_cols=0, project_w=True,
                 verbose=False, fetch=True):
        """``ricadi_ric_radi``: low-rank RADI for the projected Riccati equation on host panels.  Returns
        ``(Z, K, info)``: the factor (``None`` with ``fetch=False``: it stays in the context), the gain
        ``cal E X B`` and the statistics (``info['stop_rule']`` is ``'res'`` or ``'max_steps'``)."""
        B = as_panel(B, self.nv)
        W = as_panel(W, self.nv)
        sh = np.ascontiguousarray(shifts, dtype=np.float64)
        nb, mw = B.shape[1], W.shape[1]
        oldB = None if oldB is None else as_panel(oldB, self.nv)
        cap = max(int(max_steps), 0) * mw
        Z = np.empty((self.nv, max(cap, 1))) if fetch else None
        K = np.zeros((self.nv, nb))
        cc = C.c_int(0)
        stats = np.zeros(8)
        self._zdev = None
        _chk(self._lib.ricadi_ric_radi(
            self._h, _d(sh), sh.size, _d(B), nb, _d(W), mw, None if oldB is None else _d(oldB), int(max_steps),
            float(res_reltol), int(compress_cols), 1 if project_w else 0, 1 if verbose else 0,
            None if Z is None else _d(Z), cap, C.byref(cc), _d(K), _d(stats)))
        c = cc.value
        if fetch:
            Z = Z.ravel()[:self.nv * c].reshape(self.nv, c)
            Z.flags.writeable = False        # as ric_newtonadi: gain(B, Z=<this array>) may use the device copy
            self._zdev = Z
        info = self._radi_info(stats, c, self.adi_stopped_by())
        _warn_nonconverged(info)
        return Z, K, info

    def ric_radi_dev(self, shifts, B_t, W_t, old_t=None, max_steps=200, res_reltol=1e-10, compress_cols=0,
                     project_w=True, verbose=False):
        """``ricadi_ric_radi_dev``: every panel is a torch CUDA tensor (float64, contiguous, NV rows); the factor and
        the gain come back as fresh CUDA tensors.  Returns ``(Zt, Kt, info)``."""
        import torch
        sh = np.ascontiguousarray(shifts, dtype=np.float64)
        for t in (B_t, W_t, old_t):
            if t is not None and not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()
                                      and t.dim() == 2 and t.shape[0] == self.nv):
                raise ValueError("device panels must be contiguous float64 CUDA tensors with NV rows")
        cc = C.c_int(0)
        stats = np.zeros(8)
        self._zdev = None
        Kt = torch.zeros_like(B_t)
        torch.cuda.current_stream().synchronize()          # the library runs on its own stream
        _chk(self._lib.ricadi_ric_radi_dev(
            self._h, _d(sh), sh.size, B_t.data_ptr(), B_t.shape[1], W_t.data_ptr(), W_t.shape[1],
            None if old_t is None else old_t.data_ptr(), int(max_steps), float(res_reltol), int(compress_cols),
            1 if project_w else 0, 1 if verbose else 0, C.byref(cc), Kt.data_ptr(), _d(stats)))
        c = cc.value
        Zt = torch.empty((self.nv, c), dtype=torch.float64, device=B_t.device)
        if c > 0:
            _chk(self._lib.ricadi_factor_get_dev(self._h, Zt.data_ptr(), c))
        info = self._radi_info(stats, c, self.adi_stopped_by())
        _warn_nonconverged(info)
        return Zt, Kt, info

    RADI_SHIFT_MODES = {"cycle": RICADI_RADI_SHIFTS_CYCLE, "hamiltonian": RICADI_RADI_SHIFTS_HAMILTONIAN,
                        "hamiltonian-dominant": RICADI_RADI_SHIFTS_HAMILTONIAN_DOMINANT}

    def set_radi_shifts(self, mode):
        """``ricadi_set_radi_shift_mode``: ``'cycle'`` (default; the list is cycled), ``'hamiltonian'`` (the list's
        first entry starts, every later shift is generated from the iteration, the list is the fallback) or
        ``'hamiltonian-dominant'`` (the same on the at most 32 dominant directions of the new block: any width).  A
        context setting, like :meth:`set_recycle`.  Returns the mode that was in force."""
        new = self.RADI_SHIFT_MODES[mode] if isinstance(mode, str) else int(mode)
        old = getattr(self, "_radi_shift_mode", RICADI_RADI_SHIFTS_CYCLE)
        _chk(self._lib.ricadi_set_radi_shift_mode(self._h, new))
        self._radi_shift_mode = new
        return old

    def set_radi_sweep_width(self, width):
        """``ricadi_set_radi_sweep_width``: how many consecutive steps of a cycled RADI run go through one lockstep
        batch of solves (1, the default: one solve per step; at most 16).  The width that runs is what the shift list
        allows (:func:`host_radi_sweep_width`).  A context setting.  Returns the width that was in force."""
        new = int(width)
        old = getattr(self, "_radi_sweep_width", 1)
        _chk(self._lib.ricadi_set_radi_sweep_width(self._h, new))
        self._radi_sweep_width = new
        return old

    def set_radi_sweep_shifts(self, on):
        """``ricadi_set_radi_sweep_shifts``: with ``'hamiltonian-dominant'`` shifts, let a sweep width above 1 run as
        sweeps whose shifts the iteration generates.  A context setting, off by default.  Returns the
        value that was in force."""
        rc = self._lib.ricadi_set_radi_sweep_shifts(self._h, int(on))
        if rc < 0:
            _chk(rc)
        return bool(rc)

    def radi_sweep_widths(self):
        """``ricadi_radi_sweep_widths``: the solves of every sweep of the last RADI call (empty after a sequential
        call)."""
        n = C.c_int(0)
        _chk(self._lib.ricadi_radi_sweep_widths(self._h, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=np.int32)
        _chk(self._lib.ricadi_radi_sweep_widths(self._h, _i(out), n.value, C.byref(n)))
        return out[:n.value].copy()

    def radi_sweep_info(self):
        """``ricadi_radi_sweep_info``: dict(width, sweeps, solves) of the last RADI call: the effective sweep width
        (with generated sweep shifts: the cap), the sweeps run (0 at width 1) and the shift solves issued."""
        out = np.zeros(3, dtype=np.int32)
        _chk(self._lib.ricadi_radi_sweep_info(self._h, _i(out)))
        return dict(width=int(out[0]), sweeps=int(out[1]), solves=int(out[2]))

    def radi_sweep_combine_dev(self, G, v_ptr, vstride, ldv, m, s_ptr, cf_ptr, k, nb, ru_ptr, z_ptr, ldz, zoff):
        """``ricadi_radi_sweep_combine_dev``: the recombination of a RADI sweep on device pointers (tests)."""
        _chk(self._lib.ricadi_radi_sweep_combine_dev(self._h, int(G), v_ptr, int(vstride), int(ldv), int(m), s_ptr,
                                                     cf_ptr, int(k), int(nb), ru_ptr, z_ptr, int(ldz), int(zoff)))

    def radi_shift_history(self):
        """``ricadi_radi_shift_history``: the shift of every step of the last RADI call (either mode)."""
        n = C.c_int(0)
        _chk(self._lib.ricadi_radi_shift_history(self._h, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1))
        _chk(self._lib.ricadi_radi_shift_history(self._h, _d(out), n.value, C.byref(n)))
        return out[:n.value].copy()

    def radi_shift_fallbacks(self):
        """``ricadi_radi_shift_fallbacks``: how many shifts of the last RADI call came from the fallback list."""
        n = C.c_int(0)
        _chk(self._lib.ricadi_radi_shift_fallbacks(self._h, C.byref(n)))
        return int(n.value)

    def cache_entries(self):
        """``ricadi_probe_cache_entries``: entries of the per-shift cache over all levels (tests)."""
        n = C.c_int(0)
        _chk(self._lib.ricadi_probe_cache_entries(self._h, C.byref(n)))
        return int(n.value)

    def probe_radi_refuse(self, steps=()):
        """``ricadi_probe_radi_refuse``: the selection after each of the listed steps (1-based) of later HAMILTONIAN
        RADI calls counts as refused; stays until replaced or cleared (an empty list).  Tests."""
        st = np.ascontiguousarray(sorted(int(v) for v in steps), dtype=np.int32)
        _chk(self._lib.ricadi_probe_radi_refuse(self._h, _i(st) if st.size else None, int(st.size)))

    def probe_radi_counters(self):
        """``ricadi_probe_radi_counters``: dict(qr_repeats, recompressions) of the last RADI call (tests)."""
        out = np.zeros(2, dtype=np.int32)
        _chk(self._lib.ricadi_probe_radi_counters(self._h, _i(out)))
        return dict(qr_repeats=int(out[0]), recompressions=int(out[1]))

    def probe_radi_kept(self):
        """``ricadi_probe_radi_kept``: the basis size of every shift selection of the last RADI call (tests)."""
        n = C.c_int(0)
        _chk(self._lib.ricadi_probe_radi_kept(self._h, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=np.int32)
        _chk(self._lib.ricadi_probe_radi_kept(self._h, _i(out), n.value, C.byref(n)))
        return out[:n.value].copy()

    def radi_reduce_dev(self, q_ptr, k, ru_ptr, m, b_ptr, nb, h_ptr):
        """``ricadi_radi_reduce_dev``: H = Q^T [cal A Q | cal E Q | R | U | B] on device pointers (tests)."""
        _chk(self._lib.ricadi_radi_reduce_dev(self._h, q_ptr, int(k), ru_ptr, int(m), b_ptr, int(nb), h_ptr))

    def radi_reduce_wide_dev(self, q_ptr, k, ru_ptr, m, b_ptr, nb, h_ptr):
        """``ricadi_radi_reduce_wide_dev``: the same on the wide kernel, k = m in 33 .. 127 (tests)."""
        _chk(self._lib.ricadi_radi_reduce_wide_dev(self._h, q_ptr, int(k), ru_ptr, int(m), b_ptr, int(nb), h_ptr))

    def radi_reduce_group_dev(self, q_ptr, c, ru_ptr, m, b_ptr, nb, h_ptr):
        """``ricadi_radi_reduce_group_dev``: the same for a group of c columns against an m-column residual (tests)."""
        _chk(self._lib.ricadi_radi_reduce_group_dev(self._h, q_ptr, int(c), ru_ptr, int(m), b_ptr, int(nb), h_ptr))

    def radi_update_dev(self, p, v_ptr, ldv, m, b_ptr, nb, ru_ptr, z_ptr, ldz, zoff, g_ptr, c_ptr=None):
        """``ricadi_radi_update_dev``: the dense part of one RADI step on device pointers (tests)."""
        _chk(self._lib.ricadi_radi_update_dev(self._h, float(p), v_ptr, int(ldv), int(m), b_ptr, int(nb), ru_ptr,
                                              z_ptr, int(ldz), int(zoff), g_ptr, c_ptr))

    def compress(self, Z=None, thresh=None, k=None):
        """``Z=None`` compresses the factor left on the device."""
        self._zdev = None
        if Z is not None:
            Z = as_panel(Z, self.nv)
            c = Z.shape[1]
        else:
            cc = C.c_int(0)
            _chk(self._lib.ricadi_factor_cols(self._h, C.byref(cc)))
            c = cc.value
        out = np.empty((self.nv, max(c, 1)))
        kk = C.c_int(0)
        sv = np.zeros(max(c, 1))
        _chk(self._lib.ricadi_compress(self._h, None if Z is None else _d(Z), c,
                                       -1.0 if thresh is None else float(thresh),
                                       0 if k is None else int(k), _d(out), C.byref(kk), _d(sv)))
        kk = kk.value
        return out.ravel()[:self.nv * kk].reshape(self.nv, kk).copy(), sv[:min(c, self.nv)]

    def recompress(self, Z, rel=0.0):
        """The drivers' internal recompression (pivoted Cholesky of the Gram matrix, no eigensolver):
        ``Zc`` with ``Zc Zc^T = Z Z^T`` up to ``rel^2 ||Z Z^T||`` (``rel=0``: the drivers' own level)."""
        Z = as_panel(Z, self.nv)
        c = Z.shape[1]
        out = np.empty((self.nv, c))
        kk = C.c_int(0)
        _chk(self._lib.ricadi_recompress(self._h, _d(Z), c, float(rel), _d(out), C.byref(kk)))
        kk = kk.value
        return out.ravel()[:self.nv * kk].reshape(self.nv, kk).copy()

    def gain(self, B, Z=None, MT=None):
        """``MT (Z (Z^T B))`` with ``MT`` = calE of the context when None."""
        B = as_panel(B, self.nv)
        K = np.empty_like(B)
        if Z is not None and Z is getattr(self, "_zdev", None) and not Z.flags.writeable:
            Z = None          # the device-resident factor IS this array (read-only since it was returned)
        if Z is not None:
            Z = as_panel(Z, self.nv)
        c = 0 if Z is None else Z.shape[1]
        if MT is not None:
            rp, ci, v, sh = as_csr(MT)
            _chk(self._lib.ricadi_gain(self._h, _i(rp), _i(ci), _d(v),
                                       None if Z is None else _d(Z), c, _d(B), B.shape[1], _d(K)))
        else:
            _chk(self._lib.ricadi_gain(self._h, None, None, None,
                                       None if Z is None else _d(Z), c, _d(B), B.shape[1], _d(K)))
        return K

    def lyap_res_norm(self, Z, W):
        Z = as_panel(Z, self.nv)
        W = as_panel(W, self.nv)
        out = C.c_double(0.0)
        _chk(self._lib.ricadi_lyap_res_norm(self._h, _d(Z), Z.shape[1], _d(W), W.shape[1],
                                            C.byref(out)))
        return out.value

    def factor_get(self):
        cc = C.c_int(0)
        _chk(self._lib.ricadi_factor_cols(self._h, C.byref(cc)))
        Z = np.empty((self.nv, cc.value))
        _chk(self._lib.ricadi_factor_get(self._h, _d(Z), cc.value))
        return Z

    # -- device-pointer level (torch tensors' data_ptr()) ------------------
    def spmm_dev(self, alpha, beta, x_ptr, m, y_ptr):
        _chk(self._lib.ricadi_spmm_dev(self._h, alpha, beta, x_ptr, m, y_ptr))

    def shift_solve_dev(self, alpha, beta, r_ptr, m, x_ptr, strict=True):
        it = C.c_int(0)
        rr = np.zeros(m)
        rc = self._lib.ricadi_shift_solve_dev(self._h, alpha, beta, r_ptr, m, x_ptr,
                                              C.byref(it), _d(rr))
        _chk(rc, allow_noconv=not strict)
        return it.value, rr

    def shift_solve_batch_dev(self, alphas, betas, r_ptr, r_stride, m, x_ptr, strict=True):
        """One batched solve for the shifts ``(alphas[g], betas[g])``; the right-hand sides
        are ``r_ptr + g*r_stride`` (``r_stride = 0``: shared), the solutions the ``n x m``
        panels ``x_ptr + g*n*m``.  Returns ``(iters per group, relres (ng x m))``."""
        al = np.ascontiguousarray(alphas, dtype=np.float64)
        be = np.ascontiguousarray(betas, dtype=np.float64)
        ng = al.size
        its = (C.c_int * ng)()
        rr = np.zeros((ng, m))
        rc = self._lib.ricadi_shift_solve_batch_dev(self._h, ng, _d(al), _d(be), r_ptr,
                                                    int(r_stride), m, x_ptr, its, _d(rr))
        _chk(rc, allow_noconv=not strict)
        return list(its), rr

    # slots of ricadi_solve_trace (include/ricadi.h)
    TRACE = ("solves", "guess_tried", "guess_used", "guess_cols", "guess_rank", "guess_pan", "stored", "smw_solves",
             "smw_setups", "smw_dup", "smw_bad", "smw_refined", "inop_lowrank", "esc1_groups", "esc2_groups",
             "wide_passes", "wide_chunks", "wide_groups_last", "cycles", "cycle_len_last", "cycle_len_max",
             "stalled_groups", "maxit_groups")

    def solve_trace(self):
        """Counters of the branches the batched shift solves of this context took so far (dict; cumulative --
        take differences -- except ``guess_cols / guess_rank / guess_pan`` and the ``*_last`` ones, which describe
        the most recent event, and ``cycle_len_max``, the largest so far)."""
        a = (C.c_int64 * len(self.TRACE))()
        _chk(self._lib.ricadi_solve_trace(self._h, a, len(self.TRACE)))
        return dict(zip(self.TRACE, (int(v) for v in a)))

    def recycle_guess_dev(self, alphas, betas, r_ptr, m, x_ptr):
        """The recycled initial guess a batched solve of these shifts with the shared ``NV x m`` right-hand side
        at ``r_ptr`` would start from, into the ``n x m`` panels at ``x_ptr``; no solve, nothing stored.  Returns
        the rank of the stored columns' Gram matrix; 0: no guess, the panels are untouched."""
        al = np.ascontiguousarray(alphas, dtype=np.float64)
        be = np.ascontiguousarray(betas, dtype=np.float64)
        rank = C.c_int(0)
        _chk(self._lib.ricadi_recycle_guess_dev(self._h, al.size, _d(al), _d(be), r_ptr, int(m), x_ptr,
                                                C.byref(rank)))
        return rank.value

    def time_spmm_batch_dev(self, alphas, betas, x_ptr, m, y_ptr, reps):
        """Milliseconds per batched saddle-SpMM launch (ng panels, one shift each)."""
        al = np.ascontiguousarray(alphas, dtype=np.float64)
        be = np.ascontiguousarray(betas, dtype=np.float64)
        ms = C.c_double(0.0)
        _chk(self._lib.ricadi_time_spmm_batch_dev(self._h, al.size, _d(al), _d(be), x_ptr, m, y_ptr,
                                                  reps, C.byref(ms)))
        return ms.value

    TK = dict(spmm=0, block_v=1, block_p=2, coarse=3, spmm_sy=4, dots=5, update_dots=6, update=7,
              precond=8, restrict=9, pc_restrict=10, pc_coarse=11, pc_sy_prows=12, pc_two_term=13,
              pc_jprod=14, pc_schur=15, pc_rect=16, iter=17, iter_split=18, pc_vanka=19)

    def time_kernel_dev(self, which, alphas, betas, m, nvec=7, reps=100):
        """Milliseconds per launch of one hot-path kernel class (``Context.TK``) as the
        batched GMRES issues it for ``len(alphas)`` groups of width ``m``."""
        al = np.ascontiguousarray(alphas, dtype=np.float64)
        be = np.ascontiguousarray(betas, dtype=np.float64)
        ms = C.c_double(0.0)
        _chk(self._lib.ricadi_time_kernel_dev(self._h, int(self.TK.get(which, which)), al.size, _d(al),
                                              _d(be), int(m), int(nvec), int(reps), C.byref(ms)))
        return ms.value

    # RICADI_PROBE_* of include/ricadi.h
    PROBE = dict(basis=0, w=1, w32=2, vcur=3, h1=4, h2=5, hsum=6, H=7, cs=8, sn=9, g=10, scale=11, resid0=12,
                 resid1=13, y=14, nrm2=15, ls_coef=16, form=17)
    PROBE_FORM = ("b16", "b32", "h16", "keepw", "fuseh", "x32", "w32", "lowsync")

    def arnoldi_probe_begin_dev(self, alphas, betas, m, r_ptr, bnorm_ptr):
        """Cycle start of the step probe for ``len(alphas)`` groups of width ``m``: residual panels
        ``[ng][n][m]`` at ``r_ptr``, ``||b||`` per column ``[ng][m]`` at ``bnorm_ptr`` (device)."""
        al = np.ascontiguousarray(alphas, dtype=np.float64)
        be = np.ascontiguousarray(betas, dtype=np.float64)
        _chk(self._lib.ricadi_arnoldi_probe_begin_dev(self._h, al.size, _d(al), _d(be), int(m), r_ptr, bnorm_ptr))

    def arnoldi_probe_step_dev(self, j, w_ptr, groups):
        """The Arnoldi phase of iteration ``j`` on the FP64 panels ``[ng][n][m]`` at ``w_ptr`` for ``groups``."""
        g = (C.c_int * len(groups))(*[int(x) for x in groups])
        _chk(self._lib.ricadi_arnoldi_probe_step_dev(self._h, int(j), w_ptr, len(groups), g))

    def arnoldi_probe_close_dev(self, ks, nz, z_ptr, x_ptr):
        """Cycle end: group ``g`` with ``ks[g]`` vectors, the FP32 slots ``[nz][ng][n][m]`` at ``z_ptr``,
        ``x += Z y`` on the FP64 panels at ``x_ptr``."""
        k = (C.c_int * len(ks))(*[int(x) for x in ks])
        _chk(self._lib.ricadi_arnoldi_probe_close_dev(self._h, k, int(nz), z_ptr, x_ptr))

    def arnoldi_probe_read_dev(self, what, out_ptr, cap, slot=0):
        """Workspace array ``what`` (``Context.PROBE``) as FP64 into ``out_ptr`` (room for ``cap`` doubles);
        returns the number of doubles written."""
        cnt = C.c_int64(0)
        _chk(self._lib.ricadi_arnoldi_probe_read_dev(self._h, int(self.PROBE.get(what, what)), int(slot), out_ptr,
                                                     int(cap), C.byref(cnt)))
        return int(cnt.value)

    def setup_info(self):
        a = (C.c_int * 30)()
        _chk(self._lib.ricadi_setup_info(self._h, a, 30))
        return dict(zip(("nv", "np", "nbv", "nbp", "bs", "kc", "spmm_row_blocks", "spmm_max_cols", "levels",
                         "dense_coarse", "fp16_vector_input", "rect_ks", "two_term_ks", "np_", "nnz_j",
                         "nnz_sy", "nnz_restriction", "coarse_route", "k1_variant", "fp32_intermediate", "fp32_operator_output",
                         "child_smoother", "vanka_colours", "vanka_patches", "vanka_largest_patch", "vanka_dropped",
                         "vanka_lone_patches", "hierarchy", "hierarchy_levels", "hierarchy_dense"),
                        list(a)))

    def dense_inverse_batch(self, mats):
        """In-place inverses of a batch of dense matrices by the setup's coarse-matrix routine; returns
        (inverses, route) -- route 0 block Gauss-Jordan, 1 rocSOLVER with partial pivoting."""
        A = np.ascontiguousarray(mats, dtype=np.float64).copy()
        if A.ndim != 3 or A.shape[1] != A.shape[2]:
            raise ValueError("mats must be nb x k x k")
        route = C.c_int(-1)
        _chk(self._lib.ricadi_dense_inverse_batch(self._h, A.shape[1], A.shape[0], _d(A), C.byref(route)))
        return A, int(route.value)

    # RICADI_PCF_* of include/ricadi.h: the branch each stage of a preconditioner application took
    PCF_RESTRICT = {0: None, 1: "rowwave", 2: "csr16", 3: "csr64"}
    PCF_COARSE = {0: None, 1: "child", 2: "dense"}
    PCF_FIRST = {0: None, 1: "two32", 2: "two_term", 3: "plain"}
    PCF_LAST = {0: None, 1: "rect32", 2: "rect", 3: "csr_in"}

    @classmethod
    def decode_precond_form(cls, w):
        w &= 0xFFFFFFFF
        return dict(h16=bool(w & 1), x32=bool(w & 2), mid32=bool(w & 4), b16=bool(w & 8),
                    restrict=cls.PCF_RESTRICT[(w >> 4) & 3], coarse=cls.PCF_COARSE[(w >> 6) & 3],
                    pfused=bool(w & (1 << 8)), psplit=bool(w & (1 << 9)), first=cls.PCF_FIRST[(w >> 10) & 3],
                    last=cls.PCF_LAST[(w >> 12) & 3], folded=bool(w & (1 << 14)), vanka=bool(w & (1 << 15)),
                    two_term_ks=(w >> 16) & 255,
                    rect_ks=(w >> 24) & 255)

    def precond_apply_batch_dev(self, alphas, betas, r_ptr, r_stride, m, z_ptr, active=None):
        """``Z_g = P(alphas[g], betas[g])^-1 R_g`` as the lockstep GMRES applies it to a batch of
        ``len(alphas)`` panels of width ``m`` (``R_g = r_ptr + g*r_stride``, ``Z_g = z_ptr + g*n*m``, device
        FP64); ``active``: the group ids to apply it to (the other panels of Z are not written).  Returns the
        decoded ``form`` word (``decode_precond_form``): which branch every stage of the cycle took."""
        al = np.ascontiguousarray(alphas, dtype=np.float64)
        be = np.ascontiguousarray(betas, dtype=np.float64)
        act = None if active is None else np.ascontiguousarray(active, dtype=np.int32)
        form = C.c_int(-1)
        _chk(self._lib.ricadi_precond_apply_batch_dev(self._h, al.size, _d(al), _d(be), r_ptr, int(r_stride), int(m),
                                                      None if act is None else _i(act),
                                                      0 if act is None else act.size, z_ptr, C.byref(form)))
        return self.decode_precond_form(form.value)

    # flags of op_apply_batch_dev (RICADI_OA_* of include/ricadi.h)
    OA_X32, OA_Y32, OA_LOWRANK, OA_RESIDUAL = 1, 2, 4, 8

    def op_apply_batch_dev(self, alphas, betas, x_ptr, x_stride, m, y_ptr, y_stride, active=None, flags=0,
                           alpha=1.0, r_ptr=None, r_stride=0, beta_r=0.0):
        """``Y_g = beta_r R_g + alpha S(alphas[g], betas[g]) X_g`` as the lockstep GMRES launches the saddle product,
        on ``len(alphas)`` device FP64 panels of width ``m`` (``X_g = x_ptr + g*x_stride`` and so on, strides in
        elements); ``active``: the group ids to apply it to (the other panels of Y are not written); ``flags``:
        ``OA_*``.  Returns the kernel form that ran (``k1_variant`` of ``setup_info``)."""
        al = np.ascontiguousarray(alphas, dtype=np.float64)
        be = np.ascontiguousarray(betas, dtype=np.float64)
        act = None if active is None else np.ascontiguousarray(active, dtype=np.int32)
        var = C.c_int(-1)
        _chk(self._lib.ricadi_op_apply_batch_dev(self._h, al.size, _d(al), _d(be), x_ptr, int(x_stride), int(m),
                                                 None if act is None else _i(act), 0 if act is None else act.size,
                                                 int(flags), float(alpha), r_ptr, int(r_stride), float(beta_r),
                                                 y_ptr, int(y_stride), C.byref(var)))
        return int(var.value)

    def precond_structure(self, level=0):
        """Structure of the preconditioner cycle of ``level`` (0 this context, 1 its child level, 2 that level's
        child, ...: ``ValueError`` below the last one): dict with the
        velocity / pressure block lists (``bv_ptr``, ``bv_rows``, ``bp_ptr``, ``bp_rows``), ``aggof`` (dof ->
        coarse index), ``kc``, ``kcv``, ``kcp``, ``smoothed``, the prolongation ``P`` (scipy CSR, n x kc),
        ``child``, ``folded``, ``rect``, ``precond32`` and the aggregate sizes the level ended with (``agg_v``,
        ``agg_p``)."""
        sz = np.zeros(16, dtype=np.int32)
        nul = [None] * 8
        _chk(self._lib.ricadi_precond_structure(self._h, int(level), _i(sz), *nul))
        nv, np_, nbv, nbp, bs, kc, kcv, kcp, sa, nnzp, child, folded, rect, p32, agg_v, agg_p = (int(x) for x in sz)
        n = nv + np_
        out = dict(bv_ptr=np.zeros(nbv + 1, np.int32), bv_rows=np.zeros(nv, np.int32),
                   bp_ptr=np.zeros(nbp + 1, np.int32), bp_rows=np.zeros(np_, np.int32),
                   aggof=np.zeros(n if kc > 0 else 0, np.int32), p_rp=np.zeros(n + 1, np.int32),
                   p_ci=np.zeros(nnzp, np.int32), p_v=np.zeros(nnzp))
        ptr = lambda a: _d(a) if a.dtype == np.float64 else _i(a)   # noqa: E731
        _chk(self._lib.ricadi_precond_structure(self._h, int(level), _i(sz), *[ptr(out[k]) for k in (
            "bv_ptr", "bv_rows", "bp_ptr", "bp_rows", "aggof", "p_rp", "p_ci", "p_v")]))
        P = (sps.csr_matrix((out.pop("p_v"), out.pop("p_ci"), out.pop("p_rp")), shape=(n, kc)) if kc > 0 else None)
        if nbp == 0:
            out["bp_ptr"] = np.zeros(1, np.int32)
        out.update(nv=nv, np=np_, nbv=nbv, nbp=nbp, bs=bs, kc=kc, kcv=kcv, kcp=kcp, smoothed=bool(sa), P=P,
                   child=bool(child), folded=bool(folded), rect=bool(rect), precond32=bool(p32), agg_v=agg_v,
                   agg_p=agg_p)
        return out

    def precond_vanka(self, level=1):
        """The patches of the coloured Vanka sweep of ``level`` (a child level) as the device uses them: the dict
        of ``host_vanka_patches`` (every size 0 where the level has no Vanka sweep)."""
        return _vanka_records(lambda sz, cp, pi: self._lib.ricadi_precond_vanka(self._h, int(level), sz, cp, pi))

    def time_qr_dev(self, z_ptr, c, reps):
        ms = C.c_double(0.0)
        _chk(self._lib.ricadi_time_qr_dev(self._h, z_ptr, int(c), int(reps), C.byref(ms)))
        return ms.value

    def sweep_recombine_dev(self, G, u_ptr, m, rinv, cinv1, z_ptr, w_ptr):
        """Cauchy recombination of one sweep on the device; returns ``||Z-block||_F^2``."""
        ri = np.ascontiguousarray(rinv, dtype=np.float64)
        ci = np.ascontiguousarray(cinv1, dtype=np.float64)
        n2 = C.c_double(0.0)
        _chk(self._lib.ricadi_sweep_recombine_dev(self._h, int(G), u_ptr, m, _d(ri), _d(ci), z_ptr,
                                                  w_ptr, C.byref(n2)))
        return n2.value

    def sweep_recombine_slots_dev(self, nslot, G, u_ptr, m, coefz, coefw, z_ptr, w_ptr):
        """Recombination of one sweep from ``nslot`` gathered panels (see the header)."""
        cz = np.ascontiguousarray(coefz, dtype=np.float64)
        cw = np.ascontiguousarray(coefw, dtype=np.float64)
        if cz.shape != (nslot, G) or cw.shape != (nslot,):
            raise ValueError("coefficient tables do not match (nslot, G)")
        n2 = C.c_double(0.0)
        bn = np.zeros(int(G))
        _chk(self._lib.ricadi_sweep_recombine_slots_dev(self._h, int(nslot), int(G), u_ptr, m, _d(cz),
                                                        _d(cw), z_ptr, w_ptr, C.byref(n2), _d(bn)))
        return n2.value, bn

    def apply_e_dev(self, coef, v_ptr, m, w_ptr):
        _chk(self._lib.ricadi_apply_e_dev(self._h, coef, v_ptr, m, w_ptr))

    def lincomb_dev(self, nrows, m, coef, basis_ptr, stride, out_ptr):
        cf = np.ascontiguousarray(coef, dtype=np.float64)
        _chk(self._lib.ricadi_lincomb_dev(self._h, nrows, m, cf.size, basis_ptr, int(stride),
                                          _d(cf), out_ptr))

    def gain_dev(self, coef, z_ptr, c, ldz, b_ptr, nb, k_ptr):
        _chk(self._lib.ricadi_gain_dev(self._h, coef, z_ptr, c, ldz, b_ptr, nb, k_ptr))

    def panel_norms_dev(self, w_ptr, nrows, m):
        g = C.c_double(0.0)
        t = C.c_double(0.0)
        _chk(self._lib.ricadi_panel_norms_dev(self._h, w_ptr, nrows, m, C.byref(g), C.byref(t)))
        return g.value, t.value

    def time_spmm_dev(self, alpha, beta, x_ptr, m, y_ptr, reps):
        ms = C.c_double(0.0)
        _chk(self._lib.ricadi_time_spmm_dev(self._h, alpha, beta, x_ptr, m, y_ptr, reps,
                                            C.byref(ms)))
        return ms.value

    def time_gram_dev(self, z_ptr, c, g_ptr, reps):
        ms = C.c_double(0.0)
        _chk(self._lib.ricadi_time_gram_dev(self._h, z_ptr, c, g_ptr, reps, C.byref(ms)))
        return ms.value


def _qr(self, Z, want_q=True):
    """Thin QR by TSQR panels + block Gram-Schmidt (K5); returns (Q or None, R)."""
    Z = as_panel(Z, self.nv)
    c = Z.shape[1]
    R = np.empty((c, c))
    Q = np.empty_like(Z) if want_q else None
    _chk(self._lib.ricadi_qr(self._h, _d(Z), c, None if Q is None else _d(Q), _d(R)))
    return Q, R


Context.qr = _qr


def _project_pencil(self, Q):
    """``(H_A, H_E) = (Q^T (cal A - U V^T) Q, Q^T cal E Q)`` for an NV x k panel ``Q`` (k <= 128), on the device
    (K7); the low-rank term only if one is set.  Bitwise reproducible."""
    self._need_op()
    Q = as_panel(Q, self.nv)
    k = Q.shape[1]
    HA = np.empty((k, k))
    HE = np.empty((k, k))
    _chk(self._lib.ricadi_project_pencil(self._h, _d(Q), k, _d(HA), _d(HE)))
    return HA, HE


def _project_pencil_dev(self, q_ptr, k, ha_ptr, he_ptr):
    """Device-pointer form of :meth:`project_pencil` (``Q`` NV x k, ``H_A`` / ``H_E`` k x k, row-major)."""
    _chk(self._lib.ricadi_project_pencil_dev(self._h, q_ptr, int(k), ha_ptr, he_ptr))


Context.project_pencil = _project_pencil
Context.project_pencil_dev = _project_pencil_dev


def _cross_gram_dev(self, n, p, q, x_ptr, ldx, y_ptr, ldy, g_ptr):
    """``G = X^T Y`` (p x q, row-major) of two row-major device panels (``X`` n x p with leading dimension ``ldx``,
    ``Y`` n x q with ``ldy``; p, q <= 1024) on the FP64 matrix cores, sums in a fixed order: bitwise reproducible."""
    _chk(self._lib.ricadi_cross_gram_dev(self._h, int(n), int(p), int(q), x_ptr, int(ldx), y_ptr, int(ldy), g_ptr))


def _project_pencil_twosided_dev(self, l_ptr, rb_ptr, r, ha_ptr, he_ptr):
    """``(H_A, H_E) = (L^T (cal A - U V^T) Rb, L^T cal E Rb)`` for two NV x r device panels (r <= 128): the two-sided
    form of :meth:`project_pencil_dev`.  Bitwise reproducible."""
    self._need_op()
    _chk(self._lib.ricadi_project_pencil_twosided_dev(self._h, l_ptr, rb_ptr, int(r), ha_ptr, he_ptr))


def _lqg_balance_dev(self, zc_t, zf_t, b_t, ct_t, tol, order):
    """``ricadi_lqg_balance_dev`` on contiguous float64 CUDA tensors ``Zc`` (NV x kc), ``Zf`` (NV x kf), ``B``
    (NV x nb), ``C^T`` (NV x nc); the resident operator must be ``(cal A, cal E) = (A, M)``.  Returns
    ``(r, sigma, T_l, T_r, A_r, E_r, B_r, C_r)``: ``T_l`` / ``T_r`` CUDA tensors (NV x r), the rest ndarrays."""
    import torch
    self._need_op()
    nv = self.nv
    kc, kf, nb, nc = zc_t.shape[1], zf_t.shape[1], b_t.shape[1], ct_t.shape[1]
    for t, w in ((zc_t, kc), (zf_t, kf), (b_t, nb), (ct_t, nc)):
        if t.shape[0] != nv or not t.is_contiguous() or t.dtype != torch.float64 or not 1 <= w <= 1024:
            raise ValueError("panels must be contiguous float64 NV x w tensors, 1 <= w <= 1024")
    order = int(order) if order else 0
    rcap = min(kc, kf, nv, MAX_M, order if order > 0 else MAX_M)
    tl = torch.empty(nv * rcap, dtype=torch.float64, device=zc_t.device)
    tr = torch.empty(nv * rcap, dtype=torch.float64, device=zc_t.device)
    sig = np.zeros(min(kc, kf))
    ar, er = np.zeros(rcap * rcap), np.zeros(rcap * rcap)
    br, cr = np.zeros(rcap * nb), np.zeros(nc * rcap)
    r = C.c_int(0)
    torch.cuda.current_stream().synchronize()
    _chk(self._lib.ricadi_lqg_balance_dev(self._h, zc_t.data_ptr(), kc, zf_t.data_ptr(), kf, b_t.data_ptr(), nb,
                                          ct_t.data_ptr(), nc, float(tol), order, C.byref(r), _d(sig), tl.data_ptr(),
                                          tr.data_ptr(), _d(ar), _d(er), _d(br), _d(cr)))
    r = r.value
    return (r, sig, tl[:nv * r].view(nv, r), tr[:nv * r].view(nv, r), ar[:r * r].reshape(r, r).copy(),
            er[:r * r].reshape(r, r).copy(), br[:r * nb].reshape(r, nb).copy(), cr[:nc * r].reshape(nc, r).copy())


Context.cross_gram_dev = _cross_gram_dev
Context.project_pencil_twosided_dev = _project_pencil_twosided_dev
Context.lqg_balance_dev = _lqg_balance_dev


# ---- complex shifts (include/ricadi.h, "saddle systems at COMPLEX shifts") --------------------
MAX_MC = 8               # widest complex panel
ADI_PAIR_ROWS = 32       # velocity rows per workgroup of the pair step's kernels (PAIR_ROWS of ricadi_cplx.hip)


def adi_pair_groups(width):
    """How the pair step of the ADI packs ``width`` real columns (``m``, plus ``q`` with a low-rank term):
    ``(ng, mc)`` -- ``ceil(width / 8)`` groups of ``ceil(width / ng)`` complex columns, real column ``j`` in complex
    column ``j % mc`` of group ``j // mc``."""
    ng = -(-int(width) // MAX_MC)
    return ng, -(-int(width) // ng)


def _cplx_ptr(t, shape=None):
    """Device pointer of a contiguous complex128 CUDA tensor (through ``torch.view_as_real``)."""
    import torch
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.complex128 and t.is_contiguous()):
        raise ValueError("a contiguous complex128 CUDA tensor is required")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError("tensor of shape {0} required, got {1}".format(tuple(shape), tuple(t.shape)))
    return torch.view_as_real(t).data_ptr()


def _cplx_shifts(alphas, betas):
    al = np.atleast_1d(np.asarray(alphas, dtype=np.complex128)).ravel()
    be = np.ones(al.size) if betas is None else np.atleast_1d(np.asarray(betas, dtype=np.float64)).ravel()
    if be.size != al.size or al.size < 1:
        raise ValueError("one beta per alpha required")
    return np.ascontiguousarray(al.real), np.ascontiguousarray(al.imag), np.ascontiguousarray(be)


def _shift_solve_cplx_batch_dev(self, alphas, R_t, betas=None, X_t=None, strict=True):
    """``S(alphas[g], betas[g]) X_g = [R_g; 0]`` at complex shifts (``Re alpha <= 0``, ``alpha != 0``; ``betas``
    default 1) in one lockstep batch of ``ng = len(alphas) <= 16`` groups.  ``R_t``: complex128 CUDA tensor
    ``(NV, mc)`` -- one right-hand side for all groups -- or ``(ng, NV, mc)``, ``mc <= 8``.  Returns ``(X, iters,
    relres)``: ``X`` ``(ng, n, mc)`` complex128 on the device (``X_t`` if given), iterations per group, true relative
    residuals ``(ng, mc)``.  ``strict=False`` returns what it has when a group stops at ``gmres_maxit``."""
    import torch
    self._need_op()
    ar, ai, be = _cplx_shifts(alphas, betas)
    ng = ar.size
    shared = R_t.dim() == 2
    mc = int(R_t.shape[-1])
    _cplx_ptr(R_t, (self.nv, mc) if shared else (ng, self.nv, mc))
    if X_t is None:
        X_t = torch.empty((ng, self.n, mc), dtype=torch.complex128, device=R_t.device)
    its = (C.c_int * ng)()
    rr = np.zeros((ng, mc))
    torch.cuda.current_stream().synchronize()
    rc = self._lib.ricadi_shift_solve_cplx_batch_dev(self._h, ng, _d(ar), _d(ai), _d(be), _cplx_ptr(R_t),
                                                     0 if shared else self.nv * mc, mc,
                                                     _cplx_ptr(X_t, (ng, self.n, mc)), its, _d(rr))
    _chk(rc, allow_noconv=not strict)
    return X_t, list(its), rr


def _op_apply_cplx_batch_dev(self, alphas, X_t, betas=None, Y_t=None, active=None):
    """``Y_g = S(alphas[g], betas[g]) X_g`` on complex128 CUDA tensors ``(ng, rows, mc)`` with ``rows >= n`` (the
    group stride is ``rows * mc``; only the first n rows of a group are read / written), ``mc <= 8``; ``active``: the
    group ids to apply it to.  Returns ``(Y, variant)``, variant 1 the tiled form, 2 the CSR form."""
    import torch
    self._need_op()
    ar, ai, be = _cplx_shifts(alphas, betas)
    ng = ar.size
    if X_t.dim() != 3 or X_t.shape[0] != ng:
        raise ValueError("X must be (ng, rows, mc)")
    rows, mc = int(X_t.shape[1]), int(X_t.shape[2])
    if Y_t is None:
        Y_t = torch.zeros_like(X_t)
    act = None if active is None else np.ascontiguousarray(active, dtype=np.int32)
    var = C.c_int(-1)
    torch.cuda.current_stream().synchronize()
    _chk(self._lib.ricadi_op_apply_cplx_batch_dev(self._h, ng, _d(ar), _d(ai), _d(be), _cplx_ptr(X_t), rows * mc, mc,
                                                  None if act is None else _i(act), 0 if act is None else act.size,
                                                  _cplx_ptr(Y_t, X_t.shape), int(Y_t.shape[1]) * mc, C.byref(var)))
    return Y_t, int(var.value)


def _cplx_orth_dev(self, V_t, W_t):
    """One CGS2 step of the complex Arnoldi kernels: ``W_t`` ``(ng, n, mc)`` against the basis ``V_t`` ``(nvec, ng, n,
    mc)`` (complex128 CUDA tensors, ``n`` the resident operator's).  ``W_t`` is overwritten by the unit vectors;
    returns ``H`` ``(ng, nvec + 1, mc)`` complex128 on the device: the summed coefficients, then the norm."""
    import torch
    self._need_op()
    if V_t.dim() != 4 or W_t.dim() != 3 or tuple(V_t.shape[1:]) != tuple(W_t.shape) or W_t.shape[1] != self.n:
        raise ValueError("V must be (nvec, ng, n, mc) and W (ng, n, mc)")
    nvec, ng, n, mc = (int(s) for s in V_t.shape)
    H = torch.zeros((ng, nvec + 1, mc), dtype=torch.complex128, device=W_t.device)
    torch.cuda.current_stream().synchronize()
    _chk(self._lib.ricadi_cplx_orth_dev(self._h, ng, mc, nvec, _cplx_ptr(V_t), ng * n * mc, n * mc, _cplx_ptr(W_t),
                                        _cplx_ptr(H)))
    return H


def host_cplx_proxy(alpha):
    """``ricadi_host_cplx_proxy``: the real shift ``-2^round(log2 |alpha|)`` the complex solver preconditions
    ``alpha`` with; ValueError for ``Re alpha > 0``, ``alpha = 0`` or a value that is not finite.  Host only."""
    a = complex(alpha)
    out = C.c_double(0.0)
    _chk(load().ricadi_host_cplx_proxy(a.real, a.imag, C.byref(out)))
    return float(out.value)


# RICADI_CPROBE_* of include/ricadi.h
CPROBE = dict(V=0, hout=1, Hm=2, cs=3, sn=4, gv=5, y=6, scale=7, resid=8, nrm2=9)


def _cplx_probe_begin_dev(self, R_t, bnorm):
    """Cycle start of the complex step probe: residual panels ``R_t`` ``(ng, n, mc)`` (complex128 CUDA tensor),
    ``bnorm`` ``(ng, mc)`` host array of ``||b||`` per column."""
    import torch
    self._need_op()
    if R_t.dim() != 3:
        raise ValueError("R must be (ng, n, mc)")
    ng, n, mc = (int(s) for s in R_t.shape)
    bn = np.ascontiguousarray(bnorm, dtype=np.float64)
    if n != self.n or bn.shape != (ng, mc):
        raise ValueError("R must be (ng, n, mc) with the resident n and bnorm (ng, mc)")
    torch.cuda.current_stream().synchronize()
    _chk(self._lib.ricadi_cplx_probe_begin_dev(self._h, ng, mc, _cplx_ptr(R_t), _d(bn)))
    self._cprobe = (ng, n, mc)


def _cplx_probe_step_dev(self, j, W_t, groups):
    """The Arnoldi phase of iteration ``j`` on the panels ``W_t`` ``(ng, n, mc)`` for the listed groups."""
    import torch
    g = (C.c_int * len(groups))(*[int(x) for x in groups])
    torch.cuda.current_stream().synchronize()
    _chk(self._lib.ricadi_cplx_probe_step_dev(self._h, int(j), _cplx_ptr(W_t), len(groups), g))


def _cplx_probe_close_dev(self, ks, Z_t, X_t):
    """Cycle end: group ``g`` with ``ks[g]`` vectors, ``Z_t`` ``(nz, ng, n, mc)``; ``X_t`` ``(ng, n, mc)`` is updated
    in place (``x += Z y``)."""
    import torch
    k = (C.c_int * len(ks))(*[int(x) for x in ks])
    torch.cuda.current_stream().synchronize()
    _chk(self._lib.ricadi_cplx_probe_close_dev(self._h, k, int(Z_t.shape[0]), _cplx_ptr(Z_t), _cplx_ptr(X_t)))


def _cplx_probe_read_dev(self, what, slot=0):
    """Workspace array ``what`` (``CPROBE``) of the probe cycle as a NumPy array: ``V`` ``(ng, n, mc)``, ``hout``
    ``(ng, restart + 2, 8)``, ``Hm`` ``(ng, 8, restart, restart + 1)``, ``sn`` ``(ng, 8, restart)``, ``gv``
    ``(ng, 8, restart + 1)``, ``y`` ``(ng, restart, 8)`` complex; ``cs`` ``(ng, 8, restart)``, ``scale`` / ``nrm2``
    ``(ng, 16)``, ``resid`` ``(ng, 8)`` real."""
    import torch
    ng, n, mc = getattr(self, "_cprobe", (1, self.n, 1))       # (no begin: the entry refuses the call)
    rs = int((getattr(self, "_opts", None) or default_opts()).gmres_restart)
    shapes = dict(V=(ng, n, mc), hout=(ng, rs + 2, 8), Hm=(ng, 8, rs, rs + 1), cs=(ng, 8, rs), sn=(ng, 8, rs),
                  gv=(ng, 8, rs + 1), y=(ng, rs, 8), scale=(ng, 16), resid=(ng, 8), nrm2=(ng, 16))
    real = what in ("cs", "scale", "resid", "nrm2")
    cap = int(np.prod(shapes[what])) * (1 if real else 2)
    buf = torch.full((cap,), float("nan"), dtype=torch.float64, device="cuda:0")
    cnt = C.c_int64(0)
    torch.cuda.current_stream().synchronize()
    _chk(self._lib.ricadi_cplx_probe_read_dev(self._h, int(CPROBE[what]), int(slot), buf.data_ptr(), cap, C.byref(cnt)))
    if int(cnt.value) != cap:
        raise RuntimeError("probe array {0}: {1} doubles, expected {2}".format(what, cnt.value, cap))
    a = buf.cpu().numpy()
    return a.reshape(shapes[what]).copy() if real else a.view(np.complex128).reshape(shapes[what]).copy()


Context.cplx_probe_begin_dev = _cplx_probe_begin_dev
Context.cplx_probe_step_dev = _cplx_probe_step_dev
Context.cplx_probe_close_dev = _cplx_probe_close_dev
Context.cplx_probe_read_dev = _cplx_probe_read_dev
Context.shift_solve_cplx_batch_dev = _shift_solve_cplx_batch_dev
Context.op_apply_cplx_batch_dev = _op_apply_cplx_batch_dev
Context.cplx_orth_dev = _cplx_orth_dev
Context.host_cplx_proxy = staticmethod(host_cplx_proxy)


def host_lqg_balance(S, tol=1e-12, order=0):
    """``ricadi_host_lqg_balance``: the host step of the square-root balancing, ``S = Zc^T M Zf`` (kc x kf) -> ``(r,
    sigma, coefL, coefR)`` with ``sigma`` all singular values (descending), ``r = #{sigma_i > tol sigma_1}`` capped by
    ``order`` (0: no cap), ``coefL = U_r Sigma_r^-1/2`` (kc x r), ``coefR = V_r Sigma_r^-1/2`` (kf x r); host only.
    ValueError for a bad argument or an ``S`` that is not finite, RuntimeError for ``S = 0``."""
    S = np.ascontiguousarray(S, dtype=np.float64)
    if S.ndim != 2 or S.size == 0:
        raise ValueError("S must be a non-empty matrix")
    kc, kf = S.shape
    order = int(order) if order else 0
    rcap = min(kc, kf, order) if order > 0 else min(kc, kf)
    sig, cl, cr = np.zeros(min(kc, kf)), np.zeros(kc * rcap), np.zeros(kf * rcap)
    r = C.c_int(0)
    rc = load().ricadi_host_lqg_balance(kc, kf, _d(S), float(tol), order, C.byref(r), _d(sig), _d(cl), _d(cr))
    _chk(rc)
    r = r.value
    return r, sig, cl[:kc * r].reshape(kc, r).copy(), cr[:kf * r].reshape(kf, r).copy()


def _vanka_records(call):
    sz = np.zeros(8, dtype=np.int32)
    _chk(call(_i(sz), None, None))
    ncol, npat = int(sz[0]), int(sz[1])
    cp = np.zeros(ncol + 1, dtype=np.int32)
    idx = np.full((npat, 64), -1, dtype=np.int32)
    _chk(call(_i(sz), _i(cp), _i(idx)))
    return dict(colours=ncol, patches=npat, pressure_patches=int(sz[2]), largest=int(sz[3]), dropped=int(sz[4]),
                lone=int(sz[5]), lone_patches=int(sz[6]), colour_ptr=cp, patch_idx=idx)


def host_vanka_patches(nv, J):
    """Patches and colours of the coloured Vanka sweep for a level with ``nv`` velocity unknowns and the
    constraint matrix ``J`` (np x nv; every STORED entry counts, also an explicit zero), computed on the host
    (``ricadi_host_vanka_patches``; no GPU): dict with ``colours``, ``patches`` (lone pseudo-patches included),
    ``pressure_patches``, ``largest``, ``dropped``, ``lone``, ``lone_patches``, ``colour_ptr`` (first patch of
    every colour) and ``patch_idx`` (patches x 64, -1 padded, colour by colour)."""
    J = sps.csr_matrix(J, dtype=np.float64)
    if J.shape[1] != nv:
        raise ValueError("J has the wrong number of columns")
    rp = np.ascontiguousarray(J.indptr, dtype=np.int32)
    ci = np.ascontiguousarray(J.indices, dtype=np.int32)
    v = np.ascontiguousarray(J.data, dtype=np.float64)
    lib = load()
    return _vanka_records(lambda sz, cp, pi: lib.ricadi_host_vanka_patches(int(nv), J.shape[0], _i(rp), _i(ci),
                                                                           _d(v), sz, cp, pi))


def host_aggregate(pattern, bsize):
    """Greedy BFS aggregation (host logic of the preconditioner setup)."""
    rp, ci, _, sh = as_csr(pattern)
    blk = np.empty(sh[0], dtype=np.int32)
    nb = load().ricadi_host_aggregate(sh[0], _i(rp), _i(ci), int(bsize), _i(blk))
    if nb < 0:
        _chk(nb)
    return blk, nb


def host_deal(shifts, world):
    """Owner rank of every shift of an ADI shift list (``ricadi_host_deal``)."""
    sh = np.ascontiguousarray(shifts, dtype=np.float64)
    owner = np.empty(sh.size, dtype=np.int32)
    _chk(load().ricadi_host_deal(_d(sh), sh.size, int(world), _i(owner)))
    return owner


def host_cauchy(shifts):
    """``(R^-1, C^-1 1)`` of the Cauchy matrix of a shift sweep."""
    sh = np.ascontiguousarray(shifts, dtype=np.float64)
    g = sh.size
    rinv = np.empty((g, g))
    c1 = np.empty(g)
    _chk(load().ricadi_host_cauchy(_d(sh), g, _d(rinv), _d(c1)))
    return rinv, c1


def host_adi_window_width(shifts, first, g):
    """``ricadi_host_adi_window_width``: the width the sweep form of the ADI runs for the window of ``g`` shifts
    behind step ``first`` of the cycled list (``g`` halved until ``ricadi_host_cauchy`` takes it); host only."""
    sh = np.ascontiguousarray(shifts, dtype=np.float64)
    w = C.c_int(0)
    _chk(load().ricadi_host_adi_window_width(_d(sh), int(sh.size), int(first), int(g), C.byref(w)))
    return int(w.value)


def host_radi_shift(k, m, nb, H, eigs=False):
    """``ricadi_host_radi_shift``: the next RADI shift from H = Q^T [cal A Q | cal E Q | R | U | B]
    (k x (2k + m + 2nb)); host only.  Returns ``(p, margin)`` -- p = 0.0 without a candidate --, with ``eigs`` also
    the 2k eigenvalues of the projected Hamiltonian.  ValueError for bad sizes, RuntimeError on a breakdown."""
    H = np.ascontiguousarray(H, dtype=np.float64)
    k, m, nb = int(k), int(m), int(nb)
    if min(k, m, nb) >= 1 and H.size != k * (2 * k + m + 2 * nb):       # (sizes out of range: the library says so)
        raise ValueError("H must be k x (2k + m + 2nb)")
    p, mg = C.c_double(0.0), C.c_double(0.0)
    if not eigs:
        _chk(load().ricadi_host_radi_shift(int(k), int(m), int(nb), _d(H), C.byref(p), C.byref(mg)))
        return p.value, mg.value
    wr, wi = np.zeros(2 * max(int(k), 1)), np.zeros(2 * max(int(k), 1))
    _chk(load().ricadi_host_radi_shift_eigs(int(k), int(m), int(nb), _d(H), C.byref(p), C.byref(mg), _d(wr), _d(wi)))
    return p.value, mg.value, wr + 1j * wi


RADI_REFUSALS = {1: "r_not_finite", 2: "r_zero", 3: "breakdown", 4: "no_shift"}      # RICADI_RADI_REFUSED_*


def host_radi_next_shift(m, nb, H, R, dominant=False):
    """``ricadi_host_radi_next_shift``: what the RADI driver does with what a step has fetched -- H = Q^T [cal A Q |
    cal E Q | R | U | B] for all m columns of the block's Q (m x (3m + 2nb)) and R of its QR (m x m); host only.
    Returns ``(p, margin, kept, refusal)``: ``refusal`` is None and p, margin are set, or it is one of
    ``RADI_REFUSALS``' names and p, margin are None (the driver then falls back to its list).  ``kept``: the size of the
    basis of the selection.  ValueError for bad sizes.  ``dominant``: ``ricadi_host_radi_next_shift_dominant`` -- the
    basis is the at most 32 dominant left singular directions of R (m <= 127)."""
    H = np.ascontiguousarray(H, dtype=np.float64)
    R = np.ascontiguousarray(R, dtype=np.float64)
    m, nb = int(m), int(nb)
    if min(m, nb) >= 1 and (H.size != m * (3 * m + 2 * nb) or R.size != m * m):
        raise ValueError("H must be m x (3m + 2nb) and R m x m")
    p, mg, kept = C.c_double(0.0), C.c_double(0.0), C.c_int(0)
    fn = load().ricadi_host_radi_next_shift_dominant if dominant else load().ricadi_host_radi_next_shift
    rc = fn(m, nb, _d(H), _d(R), C.byref(p), C.byref(mg), C.byref(kept))
    if rc < 0:
        _chk(rc)
    if rc > 0:
        return None, None, kept.value, RADI_REFUSALS[rc]
    return p.value, mg.value, kept.value, None


def host_radi_sweep_shifts(c, m, nb, H, R, want):
    """``ricadi_host_radi_sweep_shifts``: the shifts of the next sweep of a RADI run with generated sweep shifts, from
    what a sweep has fetched -- H = Q^T [cal A Q | cal E Q | R | U | B] for the c columns of the group's Q
    (c x (2c + m + 2nb)) and R of its QR (c x c); host only.  Returns ``(ps, crit, kept, refusal)``: the admitted shifts
    in acceptance order (at most ``want``) and their criteria, the size of the basis, and None or one of
    ``RADI_REFUSALS``' names (ps and crit are then empty).  ValueError for bad sizes."""
    H = np.ascontiguousarray(H, dtype=np.float64)
    R = np.ascontiguousarray(R, dtype=np.float64)
    c, m, nb, want = int(c), int(m), int(nb), int(want)
    if min(c, m, nb) >= 1 and (H.size != c * (2 * c + m + 2 * nb) or R.size != c * c):
        raise ValueError("H must be c x (2c + m + 2nb) and R c x c")
    ps, crit = np.zeros(max(want, 1)), np.zeros(max(want, 1))
    n, kept = C.c_int(0), C.c_int(0)
    rc = load().ricadi_host_radi_sweep_shifts(c, m, nb, _d(H), _d(R), want, _d(ps), _d(crit), C.byref(n),
                                              C.byref(kept))
    if rc < 0:
        _chk(rc)
    if rc > 0:
        return np.zeros(0), np.zeros(0), kept.value, RADI_REFUSALS[rc]
    return ps[:n.value].copy(), crit[:n.value].copy(), kept.value, None


def host_radi_sweep(shifts, m, nb, Ghat, Gamma, rhs, res_reltol, steps_left):
    """``ricadi_host_radi_sweep``: what the RADI driver does with what a sweep has fetched -- the g shifts, Ghat = Vh^T B
    (g m x nb) and Gamma, the Gram matrix of [R_0 | cal E Vh] ((g + 1) m square); host only.  Returns ``(k, res, Cf)``:
    the steps kept, the relative residual after each, and Cf = [T_k | T_k y | T_k h] (g m x (k m + m + nb)).
    ValueError for bad sizes, RuntimeError on a breakdown."""
    sh = np.ascontiguousarray(shifts, dtype=np.float64)
    Ghat = np.ascontiguousarray(Ghat, dtype=np.float64)
    Gamma = np.ascontiguousarray(Gamma, dtype=np.float64)
    g, m, nb = int(sh.size), int(m), int(nb)
    if min(g, m, nb) >= 1 and (Ghat.size != g * m * nb or Gamma.size != ((g + 1) * m) ** 2):
        raise ValueError("Ghat must be g m x nb and Gamma (g + 1) m square")
    k = C.c_int(0)
    res = np.zeros(max(g, 1))
    Cf = np.zeros(max(g * m, 1) * (max(g * m, 1) + max(m, 1) + max(nb, 1)))
    _chk(load().ricadi_host_radi_sweep(g, m, nb, _d(sh), _d(Ghat), _d(Gamma), float(rhs), float(res_reltol),
                                       int(steps_left), C.byref(k), _d(res), _d(Cf)))
    kk = k.value
    ldc = kk * m + m + nb
    return kk, res[:kk].copy(), Cf[:g * m * ldc].reshape(g * m, ldc).copy()


def host_radi_sweep_width(shifts, mw, nb, want, max_steps):
    """``ricadi_host_radi_sweep_width``: the sweep width a cycled RADI run takes for this list (1: one solve per
    step); host only."""
    sh = np.ascontiguousarray(shifts, dtype=np.float64)
    w = C.c_int(0)
    _chk(load().ricadi_host_radi_sweep_width(_d(sh), int(sh.size), int(mw), int(nb), int(want), int(max_steps),
                                             C.byref(w)))
    return int(w.value)


def host_plan_levels(calA, calE, J, **opts):
    """The preconditioner hierarchy ``set_operator`` would choose (``ricadi_host_plan_levels``; host only):
    dict(levels, kc, kcv, kcp, smoothed)."""
    a, e, j = as_csr(calA), as_csr(calE), as_csr(J)
    o = default_opts(**opts)
    out = np.zeros(5, dtype=np.int32)
    _chk(load().ricadi_host_plan_levels(a[3][0], j[3][0], _i(a[0]), _i(a[1]), _d(a[2]), _i(e[0]), _i(e[1]), _d(e[2]),
                                        _i(j[0]), _i(j[1]), _d(j[2]), C.byref(o), _i(out)))
    return dict(levels=int(out[0]), kc=int(out[1]), kcv=int(out[2]), kcp=int(out[3]), smoothed=bool(out[4]))


PLAN_KEYS = ("nv", "np", "kv", "kp", "agg_v", "agg_p", "has_child", "dense_dim")
MAX_HIERARCHY_LEVELS = 6


def host_plan_hierarchy(calA, calE, J, **opts):
    """The whole hierarchy ``set_operator`` would build, level by level (``ricadi_host_plan_hierarchy``; host only):
    a list with one dict per level -- ``nv``, ``np``, the aggregates ``kv`` / ``kp``, their sizes ``agg_v`` /
    ``agg_p``, ``has_child``, ``dense_dim`` (``kv + kp`` on the last level, 0 above it) and ``smoothed``.  A level is
    a grid with a sweep of its own: ``host_plan_levels`` counts the dense coarse problem as one level more."""
    a, e, j = as_csr(calA), as_csr(calE), as_csr(J)
    o = default_opts(**opts)
    nlev = np.zeros(1, dtype=np.int32)
    rows = np.zeros((MAX_HIERARCHY_LEVELS, 8), dtype=np.int32)
    sa = np.zeros(MAX_HIERARCHY_LEVELS, dtype=np.int32)
    _chk(load().ricadi_host_plan_hierarchy(a[3][0], j[3][0], _i(a[0]), _i(a[1]), _d(a[2]), _i(e[0]), _i(e[1]),
                                           _d(e[2]), _i(j[0]), _i(j[1]), _d(j[2]), C.byref(o), _i(nlev), _i(rows),
                                           _i(sa)))
    return [dict(zip(PLAN_KEYS, (int(x) for x in rows[l])), smoothed=bool(sa[l])) for l in range(int(nlev[0]))]


def host_saddle_tiles(calA, calE, J, **opts):
    """The row-block tile format of the saddle SpMM that ``set_operator`` would build
    (``ricadi_host_saddle_tiles``; host only): dict with ``n``, ``nv``, ``nblk``, ``max_cols``, ``max_nnz``,
    ``nnz``, ``sb_ok``, ``ms_ok``, the tile arrays ``rows2`` (nblk x 32), ``rp2`` (nblk x 33), ``cols2``
    (nblk x max cols), ``lidx``, ``perm`` (tile order -> saddle CSR entry), the saddle CSR ``s_rp``, ``s_ci`` with
    its value sources ``src_a``, ``src_e``, ``src_j``, and with ``ms_ok`` the multi-shift operands ``lidx_ms``,
    ``vAJ``, ``vE`` (else None)."""
    a, e = as_csr(calA), as_csr(calE)
    nv = a[3][0]
    j = as_csr(J) if J is not None and J.shape[0] > 0 else None
    np_ = 0 if j is None else j[3][0]
    jargs = (None, None, None) if j is None else (_i(j[0]), _i(j[1]), _d(j[2]))
    o = default_opts(**opts)
    lib = load()
    sz = np.zeros(8, dtype=np.int32)

    def call(*arrs):
        _chk(lib.ricadi_host_saddle_tiles(nv, np_, _i(a[0]), _i(a[1]), _d(a[2]), _i(e[0]), _i(e[1]), _d(e[2]),
                                          *jargs, C.byref(o), _i(sz), *arrs))

    call(*[None] * 11)
    n, nblk, max_cols, max_nnz, nnz, sb_ok, ms_ok, nv_ = (int(x) for x in sz)
    out = dict(rows2=np.zeros((nblk, 32), np.int32), rp2=np.zeros((nblk, 33), np.int32),
               cols2=np.zeros((nblk, max(max_cols, 1)), np.int32), lidx=np.zeros(nnz, np.uint16),
               lidx_ms=np.zeros(nnz, np.uint16), vAJ=np.zeros(nnz), vE=np.zeros(nnz), perm=np.zeros(nnz, np.int32),
               s_rp=np.zeros(n + 1, np.int32), s_ci=np.zeros(nnz, np.int32), s_src=np.zeros(3 * nnz))
    u16 = lambda x: x.ctypes.data_as(_up)   # noqa: E731
    call(_i(out["rows2"]), _i(out["rp2"]), _i(out["cols2"]), u16(out["lidx"]), u16(out["lidx_ms"]), _d(out["vAJ"]),
         _d(out["vE"]), _i(out["perm"]), _i(out["s_rp"]), _i(out["s_ci"]), _d(out["s_src"]))
    src = out.pop("s_src")
    out.update(src_a=src[:nnz], src_e=src[nnz:2 * nnz], src_j=src[2 * nnz:], n=n, nv=nv_, nblk=nblk,
               max_cols=max_cols, max_nnz=max_nnz, nnz=nnz, sb_ok=bool(sb_ok), ms_ok=bool(ms_ok))
    if not ms_ok:
        out.update(lidx_ms=None, vAJ=None, vE=None)
    return out


def host_sa_criterion(calA):
    """``(on, rowsum_ratio, skew_ratio)``: whether the setup would smooth the velocity aggregates for ``calA``
    (``ricadi_host_sa_criterion``; host only)."""
    rp, ci, v, sh = as_csr(calA)
    rs, sk, on = C.c_double(0.0), C.c_double(0.0), C.c_int(0)
    _chk(load().ricadi_host_sa_criterion(sh[0], _i(rp), _i(ci), _d(v), C.byref(rs), C.byref(sk), C.byref(on)))
    return bool(on.value), rs.value, sk.value
