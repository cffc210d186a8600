"""ctypes binding of libgravhmc.so (the C-ABI of include/gravhmc.h).

There is no CPU implementation behind this module: if the shared library is missing, or
the process has no usable HIP device, the calls raise.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
#: GRAVHMC_LIB: another build of the library (A/B measurements of one kernel change on one box)
LIB_PATH = os.environ.get("GRAVHMC_LIB") or os.path.join(_HERE, "libgravhmc.so")

GH_OK, GH_ERR_ARG, GH_ERR_HIP, GH_ERR_NOMEM, GH_ERR_OVERFLOW, GH_ERR_UNSUPPORTED, GH_ERR_COMM = \
    0, -1, -2, -3, -4, -5, -6
CELL_PRISM, CELL_TESSEROID, CELL_PRISM_TF, CELL_PRISM_COMP, CELL_TESSEROID_COMP, CELL_PRISM_JOINT = 0, 1, 2, 3, 4, 5
CELL_PRISM_MULTI = 6
CELL_PRISM_MVI = 7
CELL_PRISM_MVI_DATA = 8
CELL_TESS_MVI_DATA = 9
CELL_TESSEROID_MULTI = 10
#: gh_set_translation_invariant's modes beside 0 / 1 (GH_TABLE_*): the table that takes chain batches, the bootstrap batch
TABLE_CHAINS, TABLE_REPLICATES = 2, 4
#: the magnetic data components of prisms (GH_BCOMP_*, gh_set_cells_mvi_data / gh_b_result)
BCOMP_TF, BCOMP_BX, BCOMP_BY, BCOMP_BZ = range(4)
BCOMPONENTS = {"tf": BCOMP_TF, "bx": BCOMP_BX, "by": BCOMP_BY, "bz": BCOMP_BZ}
#: data components a CELL_PRISM_MVI_DATA context stacks at most (GH_BCOMP_MAX)
BCOMP_MAX = 4
#: components a CELL_PRISM_MULTI context stacks at most (GH_MULTI_MAX)
MULTI_MAX = 11
#: the gravity fields of prisms and tesseroids (GH_COMP_*, gh_set_cells_prism / gh_set_cells_tess)
COMP_POTENTIAL, COMP_GEOID, COMP_GX, COMP_GY, COMP_GZ, COMP_GXX, COMP_GXY, COMP_GXZ, COMP_GYY, COMP_GYZ, COMP_GZZ = \
    range(11)
COMPONENTS = {"potential": COMP_POTENTIAL, "geoid": COMP_GEOID, "gx": COMP_GX, "gy": COMP_GY, "gz": COMP_GZ,
              "gxx": COMP_GXX, "gxy": COMP_GXY, "gxz": COMP_GXZ, "gyy": COMP_GYY, "gyz": COMP_GYZ, "gzz": COMP_GZZ}
REG_KINDS = {"Damping": 0, "Smoothness": 1, "MS": 2, "TV": 3}

_dp = C.POINTER(C.c_double)
_ctx = C.c_void_p
_i64 = C.c_int64

#: every symbol include/gravhmc.h declares: name -> (restype, argtypes)
PROTOTYPES = {
    "gh_create": (C.c_int, [C.POINTER(_ctx), C.c_int, _i64, _i64]),
    "gh_destroy": (None, [_ctx]),
    "gh_last_error": (C.c_char_p, [_ctx]),
    "gh_device_info": (C.c_int, [_ctx, C.c_char_p, C.POINTER(C.c_int), C.POINTER(_i64)]),
    "gh_synchronize": (C.c_int, [_ctx]),
    "gh_set_obs": (C.c_int, [_ctx, _dp, _dp, _dp]),
    "gh_set_cells": (C.c_int, [_ctx, _dp, C.c_int, C.c_double]),
    "gh_set_cells_tf": (C.c_int, [_ctx, _dp, C.c_double, C.c_double, C.c_double]),
    "gh_set_cells_joint": (C.c_int, [_ctx, _dp, C.c_double, C.c_double, C.c_double]),
    "gh_set_cells_joint_table": (C.c_int, [_ctx, _dp, C.c_double, C.c_double, C.c_double]),
    "gh_set_cells_mvi": (C.c_int, [_ctx, _dp, C.c_double, C.c_double, C.c_double]),
    "gh_set_cells_mvi_data": (C.c_int, [_ctx, _dp, C.c_double, C.c_double, C.c_double, C.c_int, C.POINTER(C.c_int), _dp]),
    "gh_b_result": (C.c_int, [_ctx, C.c_int, _dp, _dp]),
    "gh_set_cells_tess_mag": (C.c_int, [_ctx, _dp, C.c_double, C.c_int, C.POINTER(C.c_int), _dp, _dp]),
    "gh_set_cells_tess_mag_table": (C.c_int, [_ctx, _dp, C.c_double, C.c_int, C.POINTER(C.c_int), _dp, _dp]),
    "gh_tess_b_result": (C.c_int, [_ctx, C.c_int, _dp, _dp]),
    "gh_set_amplitude": (C.c_int, [_ctx, C.c_double, C.c_double, C.c_double]),
    "gh_amplitude_eval": (C.c_int, [_ctx, _dp, C.POINTER(C.c_double), _dp, _dp]),
    "gh_amplitude_last": (C.c_int, [_ctx, C.POINTER(C.c_double)]),
    "gh_set_cells_multi": (C.c_int, [_ctx, _dp, C.c_int, C.POINTER(C.c_int), _dp]),
    "gh_set_cells_mvi_table": (C.c_int, [_ctx, _dp, C.c_double, C.c_double, C.c_double, C.c_int, C.POINTER(C.c_int), _dp]),
    "gh_set_cells_multi_table": (C.c_int, [_ctx, _dp, C.c_int, C.POINTER(C.c_int), _dp]),
    "gh_set_cells_multi_table_chains": (C.c_int, [_ctx, _dp, C.c_int, C.POINTER(C.c_int), _dp]),
    "gh_batch_block_means": (C.c_int, [_ctx, _dp]),
    "gh_set_cells_tess_multi": (C.c_int, [_ctx, _dp, C.c_int, C.POINTER(C.c_int), _dp, _dp]),
    "gh_multi_info": (C.c_int, [_ctx, C.POINTER(C.c_int), C.POINTER(C.c_int), _dp, _dp, _dp]),
    "gh_joint_std": (C.c_int, [_ctx, _dp]),
    "gh_joint_layout": (C.c_int, [_ctx, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gh_set_cross_gradient": (C.c_int, [_ctx, C.c_double, _dp, C.POINTER(C.c_int), C.c_double, C.c_double, _dp]),
    "gh_cross_gradient_eval": (C.c_int, [_ctx, _dp, C.POINTER(C.c_double), _dp, _dp]),
    "gh_cross_gradient_last": (C.c_int, [_ctx, C.POINTER(C.c_double)]),
    "gh_sweep_layout": (C.c_int, [_ctx, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                  C.POINTER(C.c_int), C.POINTER(_i64), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gh_tf_result": (C.c_int, [_ctx, _dp, _dp]),
    "gh_set_cells_prism": (C.c_int, [_ctx, _dp, C.c_int]),
    "gh_set_cells_tess": (C.c_int, [_ctx, _dp, C.c_int, C.c_double]),
    "gh_prism_result": (C.c_int, [_ctx, _dp, _dp]),
    "gh_set_matrix_free": (C.c_int, [_ctx, C.c_int]),
    "gh_set_matrix_free_exact": (C.c_int, [_ctx, C.c_int]),
    "gh_batch_fused_stats": (C.c_int, [_ctx, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int64),
                                       C.POINTER(C.c_int)]),
    "gh_matrix_free_team_stats": (C.c_int, [_ctx, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int64),
                                            C.POINTER(C.c_int)]),
    "gh_batch_resident_stats": (C.c_int, [_ctx, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                          C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "gh_set_shift_invariant": (C.c_int, [_ctx, C.c_int]),
    "gh_shift_invariant_info": (C.c_int, [_ctx, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                          C.POINTER(C.c_int64)]),
    "gh_pinned_alloc": (C.c_int, [_ctx, C.c_size_t, C.POINTER(C.c_void_p)]),
    "gh_pinned_free": (C.c_int, [_ctx, C.c_void_p]),
    "gh_batch_staging_stats": (C.c_int, [_ctx, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "gh_shift_invariant_resident_stats": (C.c_int, [_ctx, C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                                    C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "gh_shift_invariant_harmonic": (C.c_int, [_ctx, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int64),
                                              C.POINTER(C.c_int)]),
    "gh_shift_invariant_plan": (C.c_int, [_ctx, C.POINTER(C.c_int32)]),
    "gh_matrix_free_stats": (C.c_int, [_ctx, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64),
                                       C.POINTER(_i64), C.POINTER(_i64)]),
    "gh_build_G": (C.c_int, [_ctx]),
    "gh_kernel_stats": (C.c_int, [_ctx, C.POINTER(_i64), C.POINTER(_i64)]),
    "gh_upload_G": (C.c_int, [_ctx, _dp, _i64, C.c_int]),
    "gh_download_G": (C.c_int, [_ctx, _dp, _i64]),
    "gh_weight": (C.c_int, [_ctx, C.c_double, _dp]),
    "gh_set_data": (C.c_int, [_ctx, _dp, _dp]),
    "gh_set_reg": (C.c_int, [_ctx, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_int), _dp]),
    "gh_forward": (C.c_int, [_ctx, _dp, _dp]),
    "gh_adjoint": (C.c_int, [_ctx, _dp, _dp]),
    "gh_misfit_and_grad": (C.c_int, [_ctx, _dp, _dp, _dp, _dp]),
    "gh_reg_eval": (C.c_int, [_ctx, C.c_int, C.c_double, C.POINTER(C.c_int), C.c_int, _dp, _dp,
                              C.POINTER(C.c_double), _dp]),
    "gh_compress_wavelet": (C.c_int, [_ctx, C.c_int, C.POINTER(C.c_int), C.c_double, C.c_int,
                                      C.POINTER(_i64), C.POINTER(_i64)]),
    "gh_download_csr": (C.c_int, [_ctx, C.POINTER(_i64), C.POINTER(C.c_int32), _dp]),
    "gh_model_coeffs": (C.c_int, [_ctx, _dp, _dp]),
    "gh_forward_wavelet": (C.c_int, [_ctx, _dp, _dp]),
    "gh_chain_init": (C.c_int, [_ctx, _dp, _dp, _dp]),
    "gh_chain_trajectory": (C.c_int, [_ctx, _dp, C.c_double, C.c_int, C.c_double,
                                      C.POINTER(C.c_int), _dp]),
    "gh_chain_prefetch_momentum": (C.c_int, [_ctx, _dp]),
    "gh_chain_stats": (C.c_int, [_ctx, C.POINTER(_i64), C.POINTER(_i64)]),
    "gh_chain_resident_stats": (C.c_int, [_ctx, C.POINTER(_i64), C.POINTER(_i64)]),
    "gh_chain_resident_plan": (C.c_int, [_ctx, C.c_int, C.POINTER(C.c_int32)]),
    "gh_team_sweep_stats": (C.c_int, [_ctx, C.POINTER(C.c_int), C.POINTER(_i64), C.POINTER(C.c_int),
                                      C.POINTER(_i64)]),
    "gh_team_sweep_plan": (C.c_int, [_ctx, C.POINTER(C.c_int32)]),
    "gh_chain_run": (C.c_int, [_ctx, C.c_int, C.POINTER(C.c_int), _dp, _dp, C.c_double, _dp, _i64, _i64,
                               C.POINTER(C.c_int), _dp, _dp, C.POINTER(C.c_int)]),
    "gh_chain_feed_usable": (C.c_int, [_ctx, C.POINTER(C.c_int)]),
    "gh_chain_feed_open": (C.c_int, [_ctx, C.c_void_p, C.POINTER(C.c_int), _i64, C.c_int, C.c_int, _i64, C.c_double, _dp,
                                     C.c_double, _i64, _i64, C.c_int]),
    "gh_chain_feed_next": (C.c_int, [_ctx, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), _dp, _dp,
                                     C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gh_chain_feed_close": (C.c_int, [_ctx, C.POINTER(_i64), C.POINTER(_i64)]),
    "gh_chain_feed_stats": (C.c_int, [_ctx, _dp, _dp, _dp, C.POINTER(C.c_int)]),
    "gh_debug_feed_dry_run": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), _i64, C.c_int, C.c_int, _i64, C.c_double, _dp,
                                        _i64, C.c_int, _i64, C.POINTER(C.c_int), _dp, _dp, C.POINTER(C.c_int),
                                        C.POINTER(_i64), C.POINTER(_i64)]),
    "gh_debug_work_layout": (C.c_int, [_ctx, C.POINTER(_i64)]),
    "gh_chain_get_x": (C.c_int, [_ctx, _dp]),
    "gh_chain_get_dsyn": (C.c_int, [_ctx, _dp]),
    "gh_batch_init": (C.c_int, [_ctx, C.c_int, _dp, _dp, _dp]),
    "gh_batch_trajectory": (C.c_int, [_ctx, _dp, C.c_double, C.POINTER(C.c_int), _dp,
                                      C.POINTER(C.c_int), _dp]),
    "gh_batch_run": (C.c_int, [_ctx, C.c_int, C.POINTER(C.c_int), C.POINTER(_dp), _dp, C.c_double,
                               C.POINTER(C.c_int), _dp, _dp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gh_batch_get_x": (C.c_int, [_ctx, C.c_int, _dp]),
    "gh_bscg_run": (C.c_int, [_ctx, C.c_int, _dp, _dp, _dp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int,
                              _dp, _dp, _dp, _dp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gh_bscg_stats": (C.c_int, [_ctx, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]),
    "gh_posterior_window": (C.c_int, [_ctx, C.c_int]),
    "gh_posterior_add": (C.c_int, [_ctx]),
    "gh_posterior_read": (C.c_int, [_ctx, C.POINTER(_i64), C.POINTER(_i64), _dp, _dp]),
    "gh_posterior_stream": (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, _i64, _i64, _dp, _dp]),
    "gh_posterior_stream_slot": (C.c_int, [_ctx, C.c_int]),
    "gh_posterior_stream_add": (C.c_int, [_ctx, C.c_int, _dp]),
    "gh_posterior_stream_read": (C.c_int, [_ctx, C.POINTER(_i64), _dp, _dp, _dp, _dp, _dp, _dp]),
    "gh_posterior_stream_quantiles": (C.c_int, [_ctx, C.c_int, _dp, _dp]),
    "gh_posterior_stream_hist": (C.c_int, [_ctx, C.POINTER(C.c_uint32)]),
    "gh_posterior_stream_free": (C.c_int, [_ctx]),
    "gh_leapfrog": (C.c_int, [_ctx, _dp, _dp, C.c_double, C.c_int, _dp, _dp, C.c_double,
                              C.POINTER(C.c_int), _dp, _dp]),
    "gh_shard_unique_id": (C.c_int, [C.c_void_p]),
    "gh_shard_init": (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_int, _i64, _i64]),
    "gh_shard_init_callback": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int, C.c_int, _i64, _i64]),
    "gh_shard_init_rows": (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_int, _i64, _i64]),
    "gh_shard_init_rows_callback": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int, C.c_int, _i64, _i64]),
    "gh_shard_allreduce": (C.c_int, [_ctx, _dp, _i64]),
    "gh_rng_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32]),
    "gh_rng_destroy": (None, [C.c_void_p]),
    "gh_rng_set_threads": (C.c_int, [C.c_void_p, C.c_int]),
    "gh_host_cores": (C.c_int, []),
    "gh_rng_set_state": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_int, C.c_int, C.c_double]),
    "gh_rng_get_state": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                   C.POINTER(C.c_double)]),
    "gh_rng_draw_trajectories": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _i64, C.c_double,
                                           C.POINTER(C.c_int), _dp, _dp]),
    "gh_format_row_fixed8": (C.c_int64, [_dp, _i64, C.c_char_p, _i64]),
    "gh_measure_stream_read": (C.c_int, [_ctx, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "gh_profile_enable": (C.c_int, [_ctx, C.c_int]),
    "gh_fold_info": (C.c_int, [_ctx, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(_i64), C.POINTER(C.c_double),
                               C.POINTER(C.c_double)]),
    "gh_fold_detect": (C.c_int, [_i64, _dp, _dp, _dp, _i64, _dp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gh_fold_pair_info": (C.c_int, [_ctx, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(_i64), C.POINTER(_i64),
                                    C.POINTER(_i64)]),
    "gh_fold_detect_pair": (C.c_int, [_i64, _dp, _dp, _dp, _i64, _dp, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                      C.POINTER(C.c_int), C.POINTER(_i64), C.POINTER(C.c_int)]),
    "gh_fold_pair_rows": (C.c_int, [_i64, _dp, _dp, _dp, _i64, _dp, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                    C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(_i64), C.POINTER(C.c_int)]),
    "gh_profile_read": (C.c_int, [_ctx, C.POINTER(C.c_double), C.POINTER(_i64),
                                  C.POINTER(_i64)]),
    "gh_set_translation_invariant": (C.c_int, [_ctx, C.c_int]),
    "gh_translation_invariant_info": (C.c_int, [_ctx] + [C.POINTER(C.c_int)] * 6 + [C.POINTER(_i64), C.POINTER(C.c_double),
                                                                                   C.POINTER(C.c_double)]),
    "gh_translation_invariant_axes": (C.c_int, [_ctx] + [C.POINTER(C.c_int)] * 3),
    "gh_translation_invariant_table": (C.c_int, [_ctx, _dp]),
    "gh_translation_invariant_batch_plan": (C.c_int, [_ctx, C.POINTER(C.c_int32)]),
    "gh_lattice_detect": (C.c_int, [_i64, _dp, _dp, _dp, _i64, _dp] + [C.POINTER(C.c_int)] * 5),
}

ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, _dp, _i64)

_LIB = None


class GravHmcError(RuntimeError):
    pass


def load():
    """dlopen libgravhmc.so and bind every prototype; raises if the library is not built."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise GravHmcError(
                "libgravhmc.so is not built (%s). Run `python -m gravinv3dhmc_amd.build` "
                "(needs hipcc); there is no CPU fallback." % LIB_PATH)
        if "GRAVHMC_BATCH_TEAM" not in os.environ and not os.environ.get("GRAVHMC_LIB"):
            # batch_team_kernel covers its inline-assembly loads with hand-counted waits: the library keeps
            # that form only when the code THIS build's compiler generated for it passed the scan
            # (isa_check.py, run by build()); otherwise the two-pass batch kernels take its place
            from . import isa_check
            if not isa_check.team_form_cleared():
                import sys
                sys.stderr.write("gravinv3dhmc_amd: the generated code of batch_team_kernel was not cleared by the "
                                 "build's scan (%s): using the two-pass batch kernels\n" % isa_check.STAMP)
                os.environ["GRAVHMC_BATCH_TEAM"] = "0"
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _LIB = lib
    return _LIB


def ptr(a):
    return a.ctypes.data_as(_dp) if a is not None else None


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def check(rc, ctx=None):
    if rc == GH_OK:
        return
    msg = load().gh_last_error(ctx)
    msg = msg.decode("utf-8", "replace") if msg else "libgravhmc error %d" % rc
    if rc == GH_ERR_ARG:
        raise ValueError(msg)
    if rc == GH_ERR_OVERFLOW:
        raise OverflowError(msg)
    if rc == GH_ERR_NOMEM:
        raise MemoryError(msg)
    if rc == GH_ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    raise GravHmcError(msg)
