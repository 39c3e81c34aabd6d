"""ctypes binding of libjurassic_hip.so (include/jurassic_hip.h).

The library is the product; this module only marshals arguments.  It raises if
the shared object is missing -- there is no CPU fallback.
"""
import ctypes as C
import os
import numpy as np
from . import abi

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.environ.get("JURASSIC_HIP_SO",       # override: A/B builds
                    os.path.join(PKG, "libjurassic_hip%s.so" % os.environ.get("JUR_SUFFIX", "")))
_lib = None
dp = C.POINTER(C.c_double)


class JurassicError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(SO):
            raise JurassicError(f"{SO} not built: run `make -C jurassic-gpu_amd/csrc` "
                                "or __graft_entry__.build(); no CPU fallback exists")
        L = C.CDLL(SO)
        L.jur_last_error.restype = C.c_char_p
        L.jur_fov_read_shape.argtypes = [C.c_char_p, C.POINTER(C.c_int), dp, dp]
        L.jur_fov_apply.argtypes = [C.c_int, C.c_long, dp, dp, dp, dp, C.c_long, C.c_int, dp, dp]
        L.formod_fov.argtypes = [C.c_void_p, C.c_void_p]
        L.formod_fov.restype = None
        L.jur_tables_new.restype = C.c_void_p
        L.jur_tables_new.argtypes = [C.c_int, C.c_int]
        L.jur_tables_free.argtypes = [C.c_void_p]
        L.jur_tables_feed_rows.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_long, dp, dp, dp, dp]
        L.jur_tables_read_ascii.argtypes = [C.c_void_p, C.c_void_p]
        L.jur_tables_set_filter.argtypes = [C.c_void_p, C.c_int, C.c_int, dp, dp]
        L.jur_tables_read_filters.argtypes = [C.c_void_p, C.c_void_p]
        L.jur_tables_save.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p]
        L.jur_tables_load.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_char_p]
        L.jur_tables_cache_filename.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p]
        L.jur_tables_checksum.restype = C.c_ulonglong
        L.jur_tables_checksum.argtypes = [C.c_void_p]
        L.jur_tables_entries.restype = C.c_long
        L.jur_tables_entries.argtypes = [C.c_void_p]
        L.jur_model_create.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_int]
        L.jur_model_create_from_files.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_int]
        L.jur_model_destroy.argtypes = [C.c_void_p]
        L.jur_model_set_atm.argtypes = [C.c_void_p, C.c_void_p]
        L.jur_formod_host.argtypes = [C.c_void_p, C.c_long, C.POINTER(dp), dp, dp, C.POINTER(dp), C.POINTER(C.c_int)]
        L.jur_curtis_godson_host.argtypes = [C.c_void_p, C.c_long, C.POINTER(dp), dp, dp, dp, C.POINTER(dp), C.POINTER(C.c_int)]
        L.jur_fov_apply_device.argtypes = [C.c_void_p, C.c_long] + [C.c_void_p] * 4 + [C.c_int, dp, dp, C.c_void_p]
        L.jur_intpol_atm.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.intpol_atm.argtypes = [C.c_void_p] * 3
        L.intpol_atm.restype = None
        L.jur_host_alloc.restype = C.c_void_p
        L.jur_host_alloc.argtypes = [C.c_size_t]
        L.jur_host_free.argtypes = [C.c_void_p]
        L.jur_formod_device.argtypes = [C.c_void_p, C.c_long] + [C.c_void_p] * 7
        L.jur_formod_contrib_host.argtypes = [C.c_void_p, C.c_long, C.POINTER(dp), dp, dp, C.POINTER(dp), C.POINTER(C.c_int), dp, dp]
        L.jur_formod_contrib_device.argtypes = [C.c_void_p, C.c_long] + [C.c_void_p] * 9
        L.formod_contrib.argtypes = [C.c_void_p] * 4
        L.formod_contrib.restype = None
        L.jur_model_reserve.argtypes = [C.c_void_p, C.c_long]
        L.jur_model_workspace_bytes.restype = C.c_long
        L.jur_model_workspace_bytes.argtypes = [C.c_void_p]
        L.jur_model_table_bytes.restype = C.c_long
        L.jur_model_table_bytes.argtypes = [C.c_void_p]
        L.jur_device_info.argtypes = [C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.jur_model_chunk_rays.argtypes = [C.c_void_p]
        L.jur_model_last_launches.restype = C.c_long
        L.jur_model_last_launches.argtypes = [C.c_void_p]
        L.jur_model_set_compact_workspace.argtypes = [C.c_void_p, C.c_int]
        L.jur_model_set_chunk_rays.argtypes = [C.c_void_p, C.c_int]
        L.jur_model_set_sort_rays.argtypes = [C.c_void_p, C.c_int]
        L.jur_model_set_trace_multiple.argtypes = [C.c_void_p, C.c_int]
        L.jur_model_set_workspace_budget.argtypes = [C.c_void_p, C.c_long]
        L.jur_model_enable_timing.argtypes = [C.c_void_p, C.c_int]
        L.jur_model_last_kernel_ms.argtypes = [C.c_void_p, dp, C.POINTER(C.c_long)]
        L.jur_model_last_pencil_ms.argtypes = [C.c_void_p, dp, C.POINTER(C.c_long)]
        L.jur_model_last_contrib_ms.argtypes = [C.c_void_p, dp, C.POINTER(C.c_long)]
        L.jur_model_set_pencil.argtypes = [C.c_void_p, C.c_long, C.c_int]
        L.jur_model_set_arithmetic.argtypes = [C.c_void_p, C.c_int]
        L.jur_model_arithmetic.argtypes = [C.c_void_p]
        L.jur_multi_balance.argtypes = [C.c_void_p, C.c_long, C.POINTER(dp), C.c_int, C.POINTER(C.c_long)]
        L.jur_estimate_los_points.argtypes = [C.c_double] * 4 + [C.c_long, C.POINTER(dp), dp]
        L.jur_balance_rays.argtypes = [C.c_double] * 4 + [C.c_long, C.POINTER(dp), C.c_int, C.POINTER(C.c_long)]
        L.jur_models_set_atm.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_void_p]
        L.jur_formod_host_multi.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_long, C.POINTER(dp), dp, dp, C.POINTER(dp), C.POINTER(C.c_int)]
        L.jur_formod_device_multi.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_long, C.POINTER(C.c_long)] + [C.c_void_p] * 7
        L.jur_tune_combine.argtypes = [C.c_int, C.c_int, C.c_long]
        L.jur_tune_combine.restype = None
        L.jur_tune_trace.argtypes = [C.c_int]
        L.jur_tune_trace.restype = None
        if hasattr(L, "jur_tune_trace_slice"):       # (an older build selected with JURASSIC_HIP_SO for an A/B run has none)
            L.jur_tune_trace_slice.argtypes = [C.c_int]
            L.jur_tune_trace_slice.restype = None
        if hasattr(L, "jur_tune_block_order"):       # (likewise)
            L.jur_tune_block_order.argtypes = [C.c_int]
            L.jur_tune_block_order.restype = None
            L.jur_model_block_order.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_long]
            L.jur_model_block_order.restype = C.c_long
        if hasattr(L, "jur_tune_k_elision"):         # (likewise)
            L.jur_tune_block_order_ega.argtypes = [C.c_int]
            L.jur_tune_block_order_ega.restype = None
            L.jur_tune_k_elision.argtypes = [C.c_int]
            L.jur_tune_k_elision.restype = None
            L.jur_model_k_zero.argtypes = [C.c_void_p]
            L.jur_atm_k_zero.argtypes = [dp, C.c_long, C.c_int, C.c_int]
        L.jur_state_size.restype = C.c_size_t
        L.jur_state_size.argtypes = [C.c_void_p, C.c_void_p]
        L.jur_measurement_size.restype = C.c_size_t
        L.jur_measurement_size.argtypes = [C.c_void_p, C.c_void_p]
        L.jur_kernel.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, dp, C.c_size_t, C.c_size_t]
        ip_, lp_ = C.POINTER(C.c_int), C.POINTER(C.c_long)
        L.jur_scene_layout.argtypes = [C.c_void_p, C.c_void_p, C.c_long, dp, ip_, ip_, lp_]
        L.jur_scene_columns.restype = C.c_long
        L.jur_scene_columns.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, lp_]
        L.jur_kernel_scene_host.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(dp), dp, dp, C.POINTER(dp), ip_, lp_, dp,
                                            C.c_long]
        L.jur_model_last_scene_ms.argtypes = [C.c_void_p, dp, lp_]
        L.jur_scene_slices.restype = C.c_long
        L.jur_scene_slices.argtypes = [C.c_void_p, C.c_void_p, C.c_long, dp, ip_, ip_, ip_, lp_, lp_]
        L.jur_scene_elements.restype = C.c_long
        L.jur_scene_elements.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, lp_, ip_, ip_]
        L.jur_normal_scene_host.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(dp), dp, dp, C.POINTER(dp), ip_, lp_,
                                            dp, dp, dp, dp, dp, lp_, dp, C.c_long]
        L.jur_solve_slices_host.argtypes = [C.c_void_p, C.c_long, lp_, dp, dp, C.c_void_p, C.c_void_p]
        L.jur_step_scene_host.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(dp), dp, dp, C.POINTER(dp), ip_, lp_,
                                          dp, dp, C.c_void_p, C.c_void_p, dp, dp, dp, lp_, dp, C.c_long]
        if hasattr(L, "jur_diagnose_slices_host"):   # (likewise)
            L.jur_diagnose_slices_host.argtypes = [C.c_void_p, C.c_long, lp_, dp, dp, C.c_void_p]
            L.jur_diagnose_scene_host.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(dp), dp, dp, C.POINTER(dp), ip_, lp_,
                                                  dp, dp, dp, C.c_void_p, dp, dp, dp, lp_, dp, C.c_long]
            L.jur_avk_summary.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, dp, dp, dp, dp]
        L.jur_trial_scene_host.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(dp), dp, lp_, dp, dp, C.c_int, dp, dp, dp,
                                           dp, dp, C.c_long]
        L.jur_retrieve_decide.argtypes = [C.c_int, C.c_long, C.c_double, C.c_double, C.c_double, dp, dp, dp, ip_, dp, ip_, ip_, ip_]
        L.jur_retrieve_scene_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.POINTER(dp), dp, dp, C.POINTER(dp),
                                              ip_, lp_, dp, dp, C.c_void_p, C.c_void_p, C.c_long]
        L.jur_model_set_fov.argtypes = [C.c_void_p, C.c_int, dp, dp]
        L.jur_model_fov.argtypes = [C.c_void_p, ip_, dp, dp]
        if hasattr(L, "jur_model_set_prior_precision"):   # (an A/B library from before the full prior has none of these)
            L.jur_model_set_prior_precision.argtypes = [C.c_void_p, C.c_long, lp_, dp]
            L.jur_model_prior_precision.restype = C.c_long
            L.jur_model_prior_precision.argtypes = [C.c_void_p, lp_, dp]
            L.jur_prior_corr_host.argtypes = [C.c_void_p, C.c_long, lp_, ip_, dp, dp, C.c_int, dp, dp, dp, ip_]
        if hasattr(L, "jur_scene_hydrostatic"):
            L.jur_scene_hydrostatic.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_long, ip_, ip_, C.c_void_p]
            L.jur_scene_ray_slices.restype = C.c_long
            L.jur_scene_ray_slices.argtypes = [C.c_void_p, C.c_void_p, C.c_long, dp, ip_, ip_]
            L.jur_model_set_scene_hydz.argtypes = [C.c_void_p, C.c_double]
            L.jur_model_scene_hydz.restype = C.c_double
            L.jur_model_scene_hydz.argtypes = [C.c_void_p]
            L.jur_scene_hydrostatic_host.argtypes = [C.c_void_p, C.c_void_p, C.c_long, dp, C.c_void_p]
        L.jur_scene_fov_live.restype = C.c_long
        L.jur_scene_fov_live.argtypes = [C.c_int, C.c_long, dp, dp, C.POINTER(C.c_ubyte)]
        if hasattr(L, "jur_scene_passes"):           # (an A/B library from before the pass rules were exported has none)
            L.jur_scene_passes.restype = C.c_long
            L.jur_scene_passes.argtypes = [C.c_long, lp_, C.c_long, dp, lp_, lp_, lp_]
            L.jur_trial_passes.restype = C.c_long
            L.jur_trial_passes.argtypes = [C.c_long, C.c_int, C.c_long, dp, lp_, lp_]
            L.jur_scene_pass_reserve.argtypes = [C.c_long, lp_, C.c_long, C.c_int, dp, lp_, lp_]
        if hasattr(L, "jur_gradient_scene_host"):    # (an A/B library from before the Jacobian could be reused has none)
            L.jur_model_set_kernel_recomp.argtypes = [C.c_void_p, C.c_int]
            L.jur_model_kernel_recomp.argtypes = [C.c_void_p]
            L.jur_gradient_scene_host.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(dp), dp, dp, C.POINTER(dp), ip_, lp_,
                                                  dp, dp, dp, dp, dp, lp_, C.c_long]
            L.jur_scene_recomp_offsets.restype = C.c_long
            L.jur_scene_recomp_offsets.argtypes = [C.c_long, lp_, ip_, ip_, ip_, C.c_int, lp_]
        if hasattr(L, "jur_model_set_state_bounds"):   # (an A/B library from before the box on the state has none of these)
            L.jur_model_set_state_bounds.argtypes = [C.c_void_p, C.c_int, dp, dp]
            L.jur_model_state_bounds.argtypes = [C.c_void_p, dp, dp]
            L.jur_state_bounds_upstream.argtypes = [C.c_void_p, dp, dp]
            L.jur_state_bound.restype = C.c_double
            L.jur_state_bound.argtypes = [C.c_double, C.c_double, C.c_double]
            L.jur_state_on_bounds.restype = C.c_long
            L.jur_state_on_bounds.argtypes = [C.c_int, dp, dp, C.c_long, ip_, dp, C.POINTER(C.c_byte)]
        if hasattr(L, "jur_gain_scene_host"):        # (an A/B library from before the gain matrix has none of these)
            L.jur_gain_slices_host.argtypes = [C.c_void_p, C.c_long, lp_, dp, ip_, C.c_long, C.c_int, lp_, ip_, dp, dp, C.c_void_p,
                                               C.c_void_p]
            L.jur_gain_scene_host.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(dp), dp, dp, C.POINTER(dp), ip_, lp_,
                                              dp, dp, dp, C.c_void_p, C.c_void_p, C.c_void_p, dp, dp, dp, lp_, dp, C.c_long]
            L.jur_error_components.argtypes = [C.c_int, C.c_long, dp, dp, dp, dp, dp]
        if hasattr(L, "jur_param_slices_host"):      # (an A/B library from before the parameter errors has none of these)
            L.jur_param_slices_host.argtypes = [C.c_void_p, C.c_long, lp_, lp_, C.c_long, C.c_int, lp_, lp_, ip_, dp, dp, dp,
                                                C.c_void_p, C.c_void_p]
            L.jur_param_layout.restype = C.c_long
            L.jur_param_layout.argtypes = [C.c_long, lp_, C.c_long, lp_, lp_, ip_, lp_, lp_, lp_]
            L.jur_param_abi_sizes.argtypes = [C.POINTER(C.c_size_t)]
            L.jur_param_abi_sizes.restype = None
            L.jur_model_set_ret_windows.argtypes = [C.c_void_p, C.c_void_p]
            L.jur_model_ret_windows.argtypes = [C.c_void_p, C.c_void_p]
        if hasattr(L, "jur_param_scene_host"):       # (an A/B library from before the one-call parameter errors has none of these)
            L.jur_param_scene_host.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(dp), dp, dp, C.POINTER(dp), ip_, lp_,
                                               dp, dp, dp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, dp, dp, dp,
                                               lp_, dp, C.c_long]
            L.jur_param_scene_abi_sizes.argtypes = [C.POINTER(C.c_size_t)]
            L.jur_param_scene_abi_sizes.restype = None
            L.jur_model_scene_bytes.restype = C.c_long
            L.jur_model_scene_bytes.argtypes = [C.c_void_p]
            L.jur_model_last_cross_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double), lp_]
            L.jur_param_pass_range.argtypes = [lp_, ip_, C.c_long, C.c_long, C.c_long, lp_, lp_]
            L.jur_param_pass_range.restype = None
            L.jur_param_pass_maps.restype = C.c_long
            L.jur_param_pass_maps.argtypes = [lp_, lp_, lp_, ip_, ip_, C.c_long, C.c_long, lp_, ip_]
        if hasattr(L, "jur_model_set_scene_overflow"):   # (an A/B library from before untraceable rays were isolated has none)
            L.jur_model_set_scene_overflow.argtypes = [C.c_void_p, C.c_int]
            L.jur_model_scene_overflow.argtypes = [C.c_void_p]
            L.jur_model_last_scene_overflow.argtypes = [C.c_void_p, lp_, lp_]
            L.jur_np_overflows.argtypes = [C.c_int]
        L.jur_abi_sizes.argtypes = [C.POINTER(C.c_size_t)]
        L.jur_kat_ega_eps.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_long, dp, dp, dp, dp, C.c_int, C.c_int, dp]
        if hasattr(L, "jur_kat_cga_eps"):            # (an older build selected with JURASSIC_HIP_SO for an A/B run has none)
            L.jur_kat_cga_eps.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_long, dp, dp, dp, dp, C.c_int, C.c_int, dp]
        if hasattr(L, "jur_track_profiles"):         # (an older build selected with JURASSIC_HIP_SO for an A/B run has none)
            L.jur_track_profiles.restype = C.c_long
            L.jur_track_profiles.argtypes = [C.c_void_p, ip_, ip_, dp, ip_]
        if hasattr(L, "jur_cloud_points"):           # (an older build selected with JURASSIC_HIP_SO for an A/B run has none)
            L.jur_cloud_points.restype = C.c_long
            L.jur_cloud_points.argtypes = [C.c_void_p, dp]
            L.jur_cloud_lds_points.restype = C.c_int
            L.jur_cloud_lds_points.argtypes = []
            L.jur_kat_cloud_mean.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int, dp, dp, dp, dp]
        L.jur_kat_continua.argtypes = [C.c_void_p, C.c_int, C.c_long] + [dp] * 6
        L.jur_kat_update.argtypes = [C.c_void_p, C.c_int, C.c_long, C.c_int] + [dp] * 6
        L.jur_kat_traceray.argtypes = [C.c_void_p, C.c_long, C.POINTER(dp), dp, dp, C.POINTER(dp), C.POINTER(C.c_int)]
        for name in ("formod", "formod_GPU"):
            getattr(L, name).argtypes = [C.c_void_p] * 3
            getattr(L, name).restype = None
        L.kernel.argtypes = [C.c_void_p] * 4
        L.kernel.restype = None
        L.formod_pencil.argtypes = [C.c_void_p] * 3 + [C.c_int]
        L.formod_pencil.restype = None
        _lib = L
    return _lib


def _chk(rc):
    if rc < 0:
        raise JurassicError(f"jurassic_hip error {rc}: {lib().jur_last_error().decode()}")
    return rc


def _p(a):
    return a.ctypes.data_as(dp)


class Tables:
    def __init__(self, ng, nd):
        self.h = lib().jur_tables_new(ng, nd)
        if not self.h:
            raise JurassicError(lib().jur_last_error().decode())
        self.ng, self.nd = ng, nd

    def __del__(self):
        if getattr(self, "h", None):
            try:
                lib().jur_tables_free(self.h)
            except TypeError:          # interpreter shutdown
                pass
            self.h = None

    def feed_rows(self, ig, id_, rows):
        r = np.ascontiguousarray(rows, dtype=np.float64)
        cols = [np.ascontiguousarray(r[:, k]) for k in range(4)]
        _chk(lib().jur_tables_feed_rows(self.h, ig, id_, len(r), *[_p(c) for c in cols]))

    def read_ascii(self, ctl):
        return _chk(lib().jur_tables_read_ascii(self.h, C.byref(ctl)))

    def set_filter(self, id_, nu, f):
        nu = np.ascontiguousarray(nu, dtype=np.float64)
        f = np.ascontiguousarray(f, dtype=np.float64)
        _chk(lib().jur_tables_set_filter(self.h, id_, len(nu), _p(nu), _p(f)))

    def read_filters(self, ctl):
        _chk(lib().jur_tables_read_filters(self.h, C.byref(ctl)))

    def entries(self):
        return lib().jur_tables_entries(self.h)

    def checksum(self):
        return lib().jur_tables_checksum(self.h)

    def save(self, ctl, path):
        _chk(lib().jur_tables_save(self.h, C.byref(ctl), os.fsencode(path)))

    @classmethod
    def load(cls, ctl, path):
        h = C.c_void_p()
        _chk(lib().jur_tables_load(C.byref(h), C.byref(ctl), os.fsencode(path)))
        self = cls.__new__(cls)
        self.h, self.ng, self.nd = h, ctl.ng, ctl.nd
        return self


def _free_pinned(p):
    try:
        lib().jur_host_free(p)
    except TypeError:                  # interpreter shutdown: the module globals are gone already
        pass


class HostBuffers:
    """The arrays of one jur_formod_host call, allocated once and reused: geom (7, nr), rad/tau (nr, nd),
    tp (3, nr), np (nr,) -- in pinned host memory (jur_host_alloc) or as ordinary numpy arrays.

    A pinned block lives as long as ANY numpy view of it: the block is freed by a finalizer on the buffer object
    the arrays are views of, not by close() -- `rad = b.rad; b.close()` leaves `rad` valid."""

    def __init__(self, nr, nd, pinned=True):
        self.nr, self.nd, self.pinned = nr, nd, pinned
        self.geom = self._alloc((7, nr), np.float64)
        self.rad = self._alloc((nr, nd), np.float64)
        self.tau = self._alloc((nr, nd), np.float64)
        self.tp = self._alloc((3, nr), np.float64)
        self.np = self._alloc((nr,), np.int32)

    def _alloc(self, shape, dtype):
        if not self.pinned:
            return np.zeros(shape, dtype=dtype)
        import weakref
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = lib().jur_host_alloc(n)
        if not p:
            raise JurassicError(lib().jur_last_error().decode())
        base = (C.c_char * n).from_address(p)
        weakref.finalize(base, _free_pinned, p)          # runs when the last array that views `base` is gone
        a = np.frombuffer(base, dtype=dtype).reshape(shape)
        a[...] = 0
        return a

    def set_geometry(self, geom):
        self.geom[...] = np.asarray(geom, dtype=np.float64).T

    def close(self):
        """Drop this object's references; pinned blocks go when no array views them any more."""
        self.geom = self.rad = self.tau = self.tp = self.np = None


class Model:
    """Control block + tables resident on one GPU."""

    def __init__(self, ctl, tables=None, device=0):
        h = C.c_void_p()
        if tables is None:
            _chk(lib().jur_model_create_from_files(C.byref(h), C.byref(ctl), device))
        else:
            _chk(lib().jur_model_create(C.byref(h), C.byref(ctl), tables.h, device))
        self.h = h
        self.nd = ctl.nd
        self.ng = ctl.ng
        self.nw = ctl.nw
        self.ctl = ctl                 # (the model holds a private copy; kernel_scene lays its blocks out with this one)

    def close(self):
        if getattr(self, "h", None):
            try:
                lib().jur_model_destroy(self.h)
            except TypeError:          # interpreter shutdown: the module globals are gone already
                pass
            self.h = None

    __del__ = close

    def set_atm(self, atm):
        _chk(lib().jur_model_set_atm(self.h, C.byref(atm)))

    def set_chunk_rays(self, n):
        _chk(lib().jur_model_set_chunk_rays(self.h, n))

    def set_sort_rays(self, on):
        _chk(lib().jur_model_set_sort_rays(self.h, int(on)))

    def reserve(self, nr):
        _chk(lib().jur_model_reserve(self.h, nr))

    def set_pencil(self, max_rays, rays_per_group=0):
        """Calls of up to max_rays rays run as one fused kernel (0: never)."""
        _chk(lib().jur_model_set_pencil(self.h, max_rays, rays_per_group))

    def set_arithmetic(self, mode):
        """ARITH_FAST (default) or ARITH_EXACT: the look-up's arithmetic on strictly increasing tables."""
        _chk(lib().jur_model_set_arithmetic(self.h, int(mode)))

    def set_trace_multiple(self, mult):
        _chk(lib().jur_model_set_trace_multiple(self.h, mult))

    def k_zero(self):
        """Whether the model's next launch leaves the extinction out (jur_model_k_zero)."""
        return bool(lib().jur_model_k_zero(self.h))

    def block_order(self):
        """The block order of the last batched call (jur_model_block_order): an int32 array, empty if it built none."""
        n = lib().jur_model_block_order(self.h, None, 0)
        if n < 0:
            _chk(int(n))
        out = np.zeros(max(n, 0), dtype=np.int32)
        if n > 0 and lib().jur_model_block_order(self.h, out.ctypes.data_as(C.POINTER(C.c_int)), n) != n:
            raise RuntimeError("jur_model_block_order: the order changed between two reads")
        return out

    def set_workspace_budget(self, nbytes):
        _chk(lib().jur_model_set_workspace_budget(self.h, nbytes))

    def formod_host(self, geom, rad_in=None):
        """geom: (nr, 7).  -> dict(rad, tau, tp (nr,3), np)."""
        g = np.ascontiguousarray(np.asarray(geom, dtype=np.float64).T)
        nr, nd = g.shape[1], self.nd
        rad = np.zeros((nr, nd)) if rad_in is None else np.ascontiguousarray(rad_in, dtype=np.float64).copy()
        tau = np.zeros((nr, nd))
        tp = np.zeros((3, nr))
        npts = np.zeros(nr, dtype=np.int32)
        garr = (dp * 7)(*[_p(g[k]) for k in range(7)])
        tarr = (dp * 3)(*[_p(tp[k]) for k in range(3)])
        _chk(lib().jur_formod_host(self.h, nr, garr, _p(rad), _p(tau), tarr, npts.ctypes.data_as(C.POINTER(C.c_int))))
        return dict(rad=rad, tau=tau, tp=np.ascontiguousarray(tp.T), np=npts)

    def formod_contrib_host(self, geom, rad_in=None):
        """formod_host plus the contribution of every emitter (jur_formod_contrib_host): the formod_host dict with
        rad_c, tau_c of shape (ng + 1, nr, nd) -- [g] emitter g alone, [ng] the extinction alone."""
        g = np.ascontiguousarray(np.asarray(geom, dtype=np.float64).T)
        nr, nd = g.shape[1], self.nd
        rad = np.zeros((nr, nd)) if rad_in is None else np.ascontiguousarray(rad_in, dtype=np.float64).copy()
        tau = np.zeros((nr, nd))
        tp = np.zeros((3, nr))
        npts = np.zeros(nr, dtype=np.int32)
        rad_c = np.zeros((self.ng + 1, nr, nd))
        tau_c = np.zeros((self.ng + 1, nr, nd))
        garr = (dp * 7)(*[_p(g[k]) for k in range(7)])
        tarr = (dp * 3)(*[_p(tp[k]) for k in range(3)])
        _chk(lib().jur_formod_contrib_host(self.h, nr, garr, _p(rad), _p(tau), tarr, npts.ctypes.data_as(C.POINTER(C.c_int)),
                                           _p(rad_c), _p(tau_c)))
        return dict(rad=rad, tau=tau, tp=np.ascontiguousarray(tp.T), np=npts, rad_c=rad_c, tau_c=tau_c)

    def host_buffers(self, nr, pinned=True):
        return HostBuffers(nr, self.nd, pinned)

    def formod_host_buffers(self, b):
        """jur_formod_host on preallocated arrays (b.rad is read for the NaN mask, then overwritten)."""
        import time
        garr = (dp * 7)(*[_p(b.geom[k]) for k in range(7)])
        tarr = (dp * 3)(*[_p(b.tp[k]) for k in range(3)])
        args = (self.h, b.nr, garr, _p(b.rad), _p(b.tau), tarr, b.np.ctypes.data_as(C.POINTER(C.c_int)))
        t0 = time.perf_counter()
        rc = lib().jur_formod_host(*args)
        dt = time.perf_counter() - t0
        _chk(rc)
        return dt                                  # seconds inside the library call

    def curtis_godson(self, geom):
        """-> dict(cgp, cgt, cgu (nr, ng, NLOS), np)."""
        g = np.ascontiguousarray(np.asarray(geom, dtype=np.float64).T)
        nr = g.shape[1]
        out = [np.zeros((nr, max(self.ng, 1), abi.NLOS)) for _ in range(3)]
        npts = np.zeros(nr, dtype=np.int32)
        garr = (dp * 7)(*[_p(g[k]) for k in range(7)])
        _chk(lib().jur_curtis_godson_host(self.h, nr, garr, _p(out[0]), _p(out[1]), _p(out[2]), None,
                                          npts.ctypes.data_as(C.POINTER(C.c_int))))
        return dict(cgp=out[0], cgt=out[1], cgu=out[2], np=npts)

    def formod_device(self, nr, d_geom, d_rad, d_tau, d_tp, d_np=0, d_status=0, stream=0):
        """All arguments are raw device addresses (ints), e.g. torch_tensor.data_ptr()."""
        _chk(lib().jur_formod_device(self.h, nr, d_geom, d_rad, d_tau, d_tp, d_np, d_status, stream))

    def formod_contrib_device(self, nr, d_geom, d_rad, d_tau, d_tp, d_rad_c, d_tau_c, d_np=0, d_status=0, stream=0):
        """jur_formod_contrib_device: raw device addresses as for formod_device; d_rad_c / d_tau_c hold
        (ng + 1) x nr x nd doubles."""
        _chk(lib().jur_formod_contrib_device(self.h, nr, d_geom, d_rad, d_tau, d_tp, d_np, d_status, d_rad_c, d_tau_c, stream))

    def fov_apply_device(self, nr, d_time, d_vpz, d_rad, d_tau, dz, w, stream=0):
        """Field-of-view convolution of device arrays in place (raw device addresses as for formod_device)."""
        dz, w = (np.ascontiguousarray(a, dtype=np.float64) for a in (dz, w))
        _chk(lib().jur_fov_apply_device(self.h, nr, d_time, d_vpz, d_rad, d_tau, len(dz), _p(dz), _p(w), stream))

    def set_fov(self, dz, w=None):
        """Field of view of the scene entries (jur_model_set_fov): weights w at altitude offsets dz, as fov_read_shape
        returns them; set_fov(None) switches the convolution off.  Only kernel_scene, normal_scene, step_scene,
        trial_scene, retrieve_scene and diagnose_scene honour it."""
        if dz is None:
            _chk(lib().jur_model_set_fov(self.h, 0, None, None))
            return
        dz, w = (np.ascontiguousarray(a, dtype=np.float64).ravel() for a in (dz, w))
        if len(dz) != len(w):
            raise ValueError("dz holds %d entries, w %d" % (len(dz), len(w)))
        _chk(lib().jur_model_set_fov(self.h, len(dz), _p(dz), _p(w)))

    def fov(self):
        """The shape that is set: (dz, w), or None."""
        dz, w = np.zeros(abi.NSHAPE), np.zeros(abi.NSHAPE)
        n = C.c_int(0)
        _chk(lib().jur_model_fov(self.h, C.byref(n), _p(dz), _p(w)))
        return (dz[:n.value].copy(), w[:n.value].copy()) if n.value else None

    def set_prior_precision(self, wptr, R=None):
        """Full a-priori precision of the slices (jur_model_set_prior_precision): R flat, R_s at the running sum of the
        squared widths, [w][w], symmetric (its diagonal and lower triangle are read), laid out by wptr (nslice + 1,) as
        scene_slices lays out A; set_prior_precision(None) switches it off.  While it is set, solve_slices, step_scene,
        trial_scene, retrieve_scene, diagnose_slices and diagnose_scene take the prior as R + diag(prior_ivar) and need
        prior_ivar (it may be zeros) and its partner."""
        if wptr is None or R is None:
            _chk(lib().jur_model_set_prior_precision(self.h, 0, None, None))
            return
        wp = np.ascontiguousarray(wptr, dtype=np.int64).ravel()
        RR = np.ascontiguousarray(R, dtype=np.float64).ravel()
        ns = len(wp) - 1
        if ns < 0:
            raise ValueError("wptr must hold nslice + 1 entries")
        na = int((np.diff(wp) ** 2).sum())
        if RR.size != na:
            raise ValueError("R must hold %d doubles" % na)
        _chk(lib().jur_model_set_prior_precision(self.h, ns, wp.ctypes.data_as(C.POINTER(C.c_long)), _p(RR)))

    def prior_precision(self):
        """The precision that is set: dict(wptr, aptr, R), or None."""
        ns = _chk(lib().jur_model_prior_precision(self.h, None, None))
        if ns == 0:
            return None
        wp = np.zeros(ns + 1, dtype=np.int64)
        _chk(lib().jur_model_prior_precision(self.h, wp.ctypes.data_as(C.POINTER(C.c_long)), None))
        ap = np.concatenate(([0], np.cumsum(np.diff(wp) ** 2))).astype(np.int64)
        R = np.zeros(int(ap[-1]))
        _chk(lib().jur_model_prior_precision(self.h, None, _p(R)))
        return dict(wptr=wp, aptr=ap, R=R)

    def set_scene_hydz(self, hydz):
        """Hydrostatic balance per slice in the scene entries (jur_model_set_scene_hydz): the reference altitude [km];
        None or a negative value switches it off (the default).  While it is set kernel_scene, normal_scene, step_scene,
        trial_scene, retrieve_scene and diagnose_scene run on the atmosphere scene_hydrostatic returns and balance every
        perturbed and trial copy again (include/jurassic_hip.h)."""
        _chk(lib().jur_model_set_scene_hydz(self.h, -1.0 if hydz is None else float(hydz)))

    def scene_hydz(self):
        """The reference altitude that is set, or None."""
        v = lib().jur_model_scene_hydz(self.h)
        return v if v >= 0 else None

    def set_state_bounds(self, lo, hi=None):
        """A box on the state (jur_model_set_state_bounds): lo, hi per quantity in scene_elements' iq numbering (0 p, 1 T,
        2 + g q, 2 + ng + w k); -inf / +inf leaves a side open; lo None switches it off (the default).  While it is set
        trial_scene and retrieve_scene form state_bound(x + dx) wherever they formed x + dx; no other entry reads it."""
        if lo is None:
            _chk(lib().jur_model_set_state_bounds(self.h, 0, None, None))
            return
        l, h = (np.ascontiguousarray(v, dtype=np.float64).ravel() for v in (lo, hi))
        if len(l) != len(h):
            raise ValueError("lo and hi must have one entry per quantity each")
        _chk(lib().jur_model_set_state_bounds(self.h, len(l), _p(l), _p(h)))

    def state_bounds(self):
        """What set_state_bounds set as (lo, hi), or None."""
        nq = lib().jur_model_state_bounds(self.h, None, None)
        if nq == 0:
            return None
        lo, hi = np.zeros(nq), np.zeros(nq)
        lib().jur_model_state_bounds(self.h, _p(lo), _p(hi))
        return lo, hi

    def scene_hydrostatic(self, atm, time):
        """jur_scene_hydrostatic_host: a new atm_t, atm with p balanced on the device over the slices that rays with the
        time stamps `time` are traced through -- the atmosphere the scene entries work on while set_scene_hydz is on."""
        t = np.ascontiguousarray(time, dtype=np.float64).ravel()
        out = abi.atm_t()
        C.memmove(C.byref(out), C.byref(atm), C.sizeof(abi.atm_t))
        _chk(lib().jur_scene_hydrostatic_host(self.h, C.byref(atm), len(t), _p(t), C.byref(out)))
        return out

    def kernel(self, atm, obs):
        """Forward-difference Jacobian (m, n); obs receives the unperturbed forward model."""
        n = lib().jur_state_size(self.h, C.byref(atm))
        m = lib().jur_measurement_size(self.h, C.byref(obs))
        k = np.zeros((m, n))
        _chk(lib().jur_kernel(self.h, C.byref(atm), C.byref(obs), _p(k), m, n))
        return k

    def kernel_scene(self, atm, geom, rad_in=None, max_rays_per_pass=0, rowptr=None):
        """Block Jacobian of a scene (jur_kernel_scene_host).  geom: (nr, 7) -> the formod_host dict plus first, len
        (nr,), rowptr (nr + 1,) of scene_layout and the flat k: the block of ray r is
        k[rowptr[r] * nd : rowptr[r + 1] * nd].reshape(nd, width[r]), its columns those of scene_columns(first[r],
        len[r]).  rowptr: pass one to have it checked instead of the layout's own.
        The layout is made with the ctl_t the Model was created with, of which the model keeps a copy of its own: change
        that ctl_t afterwards (retrieval windows, say) and the call is refused with EINVAL (rowptr) -- make a new Model,
        or give the model other windows with set_ret_windows."""
        g = np.ascontiguousarray(np.asarray(geom, dtype=np.float64).T)
        nr, nd = g.shape[1], self.nd
        lay = _scene_layout(self.ctl, atm, g[0] if nr else np.zeros(0))
        rp = lay["rowptr"] if rowptr is None else np.ascontiguousarray(rowptr, dtype=np.int64)
        if rp.shape != lay["rowptr"].shape:
            raise ValueError("rowptr holds %d entries, the call has %d rays" % (len(rp), nr))
        rad = np.zeros((nr, nd)) if rad_in is None else np.ascontiguousarray(rad_in, dtype=np.float64).copy()
        tau = np.zeros((nr, nd))
        tp = np.zeros((3, nr))
        npts = np.zeros(nr, dtype=np.int32)
        k = np.zeros(int(lay["rowptr"][-1]) * nd)
        garr = (dp * 7)(*[_p(g[i]) for i in range(7)])
        tarr = (dp * 3)(*[_p(tp[i]) for i in range(3)])
        _chk(lib().jur_kernel_scene_host(self.h, C.byref(atm), nr, garr, _p(rad), _p(tau), tarr,
                                         npts.ctypes.data_as(C.POINTER(C.c_int)), rp.ctypes.data_as(C.POINTER(C.c_long)),
                                         _p(k), max_rays_per_pass))
        return dict(rad=rad, tau=tau, tp=np.ascontiguousarray(tp.T), np=npts, first=lay["first"], len=lay["len"],
                    rowptr=lay["rowptr"], k=k)

    def normal_scene(self, atm, geom, y, weight, rad_in=None, max_rays_per_pass=0, want_k=False, rowptr=None):
        """Normal equations of a scene per slice (jur_normal_scene_host).  geom: (nr, 7); y, weight: (nr, nd) -> the
        formod_host dict plus the layout (first, len, rowptr of scene_layout; sid, sfirst, slen, wptr, aptr of
        scene_slices) and the flat A, b, cost, nlive: A[aptr[s]:aptr[s + 1]].reshape(w, w), b[wptr[s]:wptr[s + 1]].
        want_k: also the blocks k as kernel_scene returns them; without it no block leaves the device.
        rowptr and the ctl_t: as kernel_scene."""
        g = np.ascontiguousarray(np.asarray(geom, dtype=np.float64).T)
        nr, nd = g.shape[1], self.nd
        time = g[0] if nr else np.zeros(0)
        lay = _scene_layout(self.ctl, atm, time)
        lay.update(scene_slices(self.ctl, atm, time))
        rp = lay["rowptr"] if rowptr is None else np.ascontiguousarray(rowptr, dtype=np.int64)
        if rp.shape != lay["rowptr"].shape:
            raise ValueError("rowptr holds %d entries, the call has %d rays" % (len(rp), nr))
        yy, ww = (np.ascontiguousarray(x, dtype=np.float64) for x in (y, weight))
        if yy.shape != (nr, nd) or ww.shape != (nr, nd):
            raise ValueError("y and weight must be (%d, %d)" % (nr, nd))
        rad = np.zeros((nr, nd)) if rad_in is None else np.ascontiguousarray(rad_in, dtype=np.float64).copy()
        tau = np.zeros((nr, nd))
        tp = np.zeros((3, nr))
        npts = np.zeros(nr, dtype=np.int32)
        ns = len(lay["sfirst"])
        A, b = np.zeros(int(lay["aptr"][-1])), np.zeros(int(lay["wptr"][-1]))
        cost, nlive = np.zeros(ns), np.zeros(ns, dtype=np.int64)
        k = np.zeros(int(lay["rowptr"][-1]) * nd) if want_k else None
        garr = (dp * 7)(*[_p(g[i]) for i in range(7)])
        tarr = (dp * 3)(*[_p(tp[i]) for i in range(3)])
        lp_ = C.POINTER(C.c_long)
        _chk(lib().jur_normal_scene_host(self.h, C.byref(atm), nr, garr, _p(rad), _p(tau), tarr,
                                         npts.ctypes.data_as(C.POINTER(C.c_int)), rp.ctypes.data_as(lp_), _p(yy), _p(ww),
                                         _p(A), _p(b), _p(cost), nlive.ctypes.data_as(lp_), _p(k) if want_k else None,
                                         max_rays_per_pass))
        out = dict(lay, rad=rad, tau=tau, tp=np.ascontiguousarray(tp.T), np=npts, A=A, b=b, cost=cost, nlive=nlive)
        if want_k:
            out["k"] = k
        return out

    def set_kernel_recomp(self, every):
        """retrieve_scene recomputes the Jacobian every `every`-th iteration (jur_model_set_kernel_recomp; 1, the default:
        in every one).  The iterations in between keep the blocks and A and renew F, b and the cost alone."""
        _chk(lib().jur_model_set_kernel_recomp(self.h, int(every)))

    def kernel_recomp(self):
        """What set_kernel_recomp set."""
        return int(lib().jur_model_kernel_recomp(self.h))

    def set_scene_overflow(self, mode):
        """What trial_scene and retrieve_scene make of a ray that needs NLOS points or more (jur_model_set_scene_overflow):
        OVERFLOW_ERROR (the default) ends the call with "Too many LOS points"; OVERFLOW_ISOLATE makes the cost of that
        trial NaN -- a rejected step -- and ends a slice whose current state cannot be traced as RET_FAILED, while every
        other slice proceeds."""
        _chk(lib().jur_model_set_scene_overflow(self.h, int(mode)))

    def scene_overflow(self):
        """What set_scene_overflow set."""
        return int(lib().jur_model_scene_overflow(self.h))

    def last_scene_overflow(self):
        """(trial cells made NaN, slices ended RET_FAILED) of the last trial_scene or retrieve_scene call
        (jur_model_last_scene_overflow); (0, 0) with OVERFLOW_ERROR."""
        a, b = C.c_long(0), C.c_long(0)
        _chk(lib().jur_model_last_scene_overflow(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def gradient_scene(self, atm, geom, y, weight, k, rad_in=None, max_rays_per_pass=0, rowptr=None):
        """Gradient and cost of a scene per slice from blocks the caller holds (jur_gradient_scene_host): the forward model
        alone, one ray per ray.  k: the flat blocks as kernel_scene returns them (None only for a state without elements)
        -> normal_scene's dict without A; with k from kernel_scene on the same atmosphere b, cost and nlive are
        normal_scene's bit for bit.  max_rays_per_pass caps the rays of a pass here."""
        g, lay, rp, yy, ww, rad = self._scene_inputs(atm, geom, y, weight, rad_in, rowptr)
        nr, nd = g.shape[1], self.nd
        nk = int(lay["rowptr"][-1]) * nd
        kk = None
        if k is not None:
            kk = np.ascontiguousarray(k, dtype=np.float64)
            if kk.shape != (nk,):
                raise ValueError("k must be the flat blocks of these rays: (%d,), not %r" % (nk, kk.shape))
        tau = np.zeros((nr, nd))
        tp = np.zeros((3, nr))
        npts = np.zeros(nr, dtype=np.int32)
        ns = len(lay["sfirst"])
        b = np.zeros(int(lay["wptr"][-1]))
        cost, nlive = np.zeros(ns), np.zeros(ns, dtype=np.int64)
        garr = (dp * 7)(*[_p(g[i]) for i in range(7)])
        tarr = (dp * 3)(*[_p(tp[i]) for i in range(3)])
        lp_ = C.POINTER(C.c_long)
        _chk(lib().jur_gradient_scene_host(self.h, C.byref(atm), nr, garr, _p(rad), _p(tau), tarr,
                                           npts.ctypes.data_as(C.POINTER(C.c_int)), rp.ctypes.data_as(lp_), _p(yy), _p(ww),
                                           _p(kk) if kk is not None else None, _p(b), _p(cost), nlive.ctypes.data_as(lp_),
                                           max_rays_per_pass))
        return dict(lay, rad=rad, tau=tau, tp=np.ascontiguousarray(tp.T), np=npts, b=b, cost=cost, nlive=nlive)

    def step_scene(self, atm, geom, y, weight, lam, mode=0, prior_ivar=None, prior_dx=None, want_normal=False, want_k=False,
                   want_factor=False, rad_in=None, max_rays_per_pass=0, rowptr=None):
        """Levenberg-Marquardt step of every slice of a scene (jur_step_scene_host): normal_scene followed by the solve
        on the device.  lam, mode, prior_ivar, prior_dx, want_factor: as solve_slices, laid out by scene_slices of these
        rays -> normal_scene's dict without A and b, plus dx (nlam, n), pred and status (nlam, nslice) and, with
        want_factor, L (nlam, aptr[-1]).  want_normal: also A and b; want_k: also the blocks.  What is not wanted never
        leaves the device."""
        g = np.ascontiguousarray(np.asarray(geom, dtype=np.float64).T)
        nr, nd = g.shape[1], self.nd
        time = g[0] if nr else np.zeros(0)
        lay = _scene_layout(self.ctl, atm, time)
        lay.update(scene_slices(self.ctl, atm, time))
        rp = lay["rowptr"] if rowptr is None else np.ascontiguousarray(rowptr, dtype=np.int64)
        if rp.shape != lay["rowptr"].shape:
            raise ValueError("rowptr holds %d entries, the call has %d rays" % (len(rp), nr))
        yy, ww = (np.ascontiguousarray(x, dtype=np.float64) for x in (y, weight))
        if yy.shape != (nr, nd) or ww.shape != (nr, nd):
            raise ValueError("y and weight must be (%d, %d)" % (nr, nd))
        rad = np.zeros((nr, nd)) if rad_in is None else np.ascontiguousarray(rad_in, dtype=np.float64).copy()
        tau = np.zeros((nr, nd))
        tp = np.zeros((3, nr))
        npts = np.zeros(nr, dtype=np.int32)
        ns, n, na = len(lay["sfirst"]), int(lay["wptr"][-1]), int(lay["aptr"][-1])
        cost, nlive = np.zeros(ns), np.zeros(ns, dtype=np.int64)
        A, b = (np.zeros(na), np.zeros(n)) if want_normal else (None, None)
        k = np.zeros(int(lay["rowptr"][-1]) * nd) if want_k else None
        sin, sout, res, keep = _solve_structs(ns, n, na, lam, mode, prior_ivar, prior_dx, want_factor)
        garr = (dp * 7)(*[_p(g[i]) for i in range(7)])
        tarr = (dp * 3)(*[_p(tp[i]) for i in range(3)])
        lp_ = C.POINTER(C.c_long)
        _chk(lib().jur_step_scene_host(self.h, C.byref(atm), nr, garr, _p(rad), _p(tau), tarr,
                                       npts.ctypes.data_as(C.POINTER(C.c_int)), rp.ctypes.data_as(lp_), _p(yy), _p(ww),
                                       C.byref(sin), C.byref(sout), _p(A) if want_normal else None,
                                       _p(b) if want_normal else None, _p(cost), nlive.ctypes.data_as(lp_),
                                       _p(k) if want_k else None, max_rays_per_pass))
        out = dict(lay, rad=rad, tau=tau, tp=np.ascontiguousarray(tp.T), np=npts, cost=cost, nlive=nlive, **res)
        if want_normal:
            out.update(A=A, b=b)
        if want_k:
            out["k"] = k
        return out

    def _scene_inputs(self, atm, geom, y, weight, rad_in, rowptr):
        """what the retrieval methods share with normal_scene: (g, layout, rowptr, y, weight, rad)"""
        g = np.ascontiguousarray(np.asarray(geom, dtype=np.float64).T)
        nr, nd = g.shape[1], self.nd
        time = g[0] if nr else np.zeros(0)
        lay = _scene_layout(self.ctl, atm, time)
        lay.update(scene_slices(self.ctl, atm, time))
        rp = lay["rowptr"] if rowptr is None else np.ascontiguousarray(rowptr, dtype=np.int64)
        if rp.shape != lay["rowptr"].shape:
            raise ValueError("rowptr holds %d entries, the call has %d rays" % (len(rp), nr))
        yy, ww = (np.ascontiguousarray(x, dtype=np.float64) for x in (y, weight))
        if yy.shape != (nr, nd) or ww.shape != (nr, nd):
            raise ValueError("y and weight must be (%d, %d)" % (nr, nd))
        rad = np.zeros((nr, nd)) if rad_in is None else np.ascontiguousarray(rad_in, dtype=np.float64).copy()
        return g, lay, rp, yy, ww, rad

    def trial_scene(self, atm, geom, y, weight, dx, prior_ivar=None, prior_xa=None, rad_in=None, max_rays_per_pass=0, rowptr=None):
        """Costs of candidate steps, forward only (jur_trial_scene_host).  dx: (ntrial, n) or (n,), laid out by
        scene_slices of these rays; prior_ivar, prior_xa (n,): both or neither -> the layout plus cost and prior
        (ntrial, nslice): cost[t, s] is normal_scene's cost of slice s on the atmosphere with dx[t] written back, bit for
        bit; prior[t, s] the prior term of that state (+0.0 without a prior)."""
        g, lay, rp, yy, ww, rad = self._scene_inputs(atm, geom, y, weight, rad_in, rowptr)
        nr = g.shape[1]
        ns, n = len(lay["sfirst"]), int(lay["wptr"][-1])
        d = np.ascontiguousarray(dx, dtype=np.float64)
        if d.ndim == 1:
            d = d.reshape(1, -1)
        if d.ndim != 2 or d.shape[1] != n:
            raise ValueError("dx must be (ntrial, %d)" % n)
        nt = d.shape[0]
        pri = [None if x is None else np.ascontiguousarray(x, dtype=np.float64).ravel() for x in (prior_ivar, prior_xa)]
        if any(x is not None and x.size != n for x in pri):
            raise ValueError("prior_ivar and prior_xa must hold %d doubles" % n)
        cost, prior = np.zeros((nt, ns)), np.zeros((nt, ns))
        garr = (dp * 7)(*[_p(g[i]) for i in range(7)])
        _chk(lib().jur_trial_scene_host(self.h, C.byref(atm), nr, garr, _p(rad), rp.ctypes.data_as(C.POINTER(C.c_long)), _p(yy),
                                        _p(ww), nt, _p(d), None if pri[0] is None else _p(pri[0]),
                                        None if pri[1] is None else _p(pri[1]), _p(cost), _p(prior), max_rays_per_pass))
        return dict(lay, cost=cost, prior=prior)

    def retrieve_scene(self, atm, geom, y, weight, max_iter, fac, lam0=1.0, lam_min=1e-6, lam_max=1e6, tol=0.0, mode=0,
                       prior_ivar=None, prior_xa=None, history=False, rad_in=None, max_rays_per_pass=0, rowptr=None,
                       atm_ret=None):
        """Retrieval of a scene on the device (jur_retrieve_scene_host): iterated Levenberg-Marquardt with trial steps,
        every slice a problem of its own.  atm_ret: an atm_t to receive the result (written only on success; it may be
        atm itself) instead of a new one.  fac (nlam,): the dampings tried per iteration are lam * fac, clamped to
        [lam_min, lam_max]; tol: a slice has converged when an accepted step lowers J = cost + prior by no more than
        tol * J; prior_ivar, prior_xa (n,): both or neither, laid out by scene_slices.
        -> the layout, "atm" (a new atm_t: atm with the retrieved elements replaced), the formod_host dict on it, x (n,),
        lam, cost, prior, nlive, state (RET_*), iters (nslice,) and, with history, h_cost, h_prior (max_iter, nslice),
        h_lam, h_tcost, h_tprior, h_status (max_iter, nlam, nslice), h_best, h_accept (max_iter, nslice) and h_work
        (max_iter, 2): the replicated rays of the Jacobian and of the trial passes.  Where a slice took no part in an
        iteration its h_lam, h_tcost, h_tprior are NaN and its h_status, h_best, h_accept -1.  Under
        set_kernel_recomp(every > 1) the iterations it % every != 0 reuse the blocks and A of the last Jacobian iteration;
        their h_work[it, 0] is the number of rays traced for the gradient.  Under set_state_bounds every trial state and
        every accepted state is state_bound(x + dx); state_on_bounds of x tells which elements the box holds.  Under
        set_scene_overflow(OVERFLOW_ISOLATE) a trial that cannot be traced has h_status TRIAL_OVERFLOW and h_tcost NaN, a
        slice whose current state cannot be traced ends RET_FAILED, and last_scene_overflow() counts both."""
        g, lay, rp, yy, ww, rad = self._scene_inputs(atm, geom, y, weight, rad_in, rowptr)
        nr, nd = g.shape[1], self.nd
        ns, n = len(lay["sfirst"]), int(lay["wptr"][-1])
        ff =np.ascontiguousarray(fac, dtype=np.float64).ravel()
        nlam, mi = len(ff), max(int(max_iter), 0)
        pri = [None if x is None else np.ascontiguousarray(x, dtype=np.float64).ravel() for x in (prior_ivar, prior_xa)]
        if any(x is not None and x.size != n for x in pri):
            raise ValueError("prior_ivar and prior_xa must hold %d doubles" % n)
        tau, tp, npts = np.zeros((nr, nd)), np.zeros((3, nr)), np.zeros(nr, dtype=np.int32)
        res = dict(x=np.zeros(n), lam=np.zeros(ns), cost=np.zeros(ns), prior=np.zeros(ns), nlive=np.zeros(ns, dtype=np.int64),
                   state=np.zeros(ns, dtype=np.int32), iters=np.zeros(ns, dtype=np.int32))
        hist = {}
        if history is True:
            hist = dict(h_cost=np.zeros((mi, ns)), h_prior=np.zeros((mi, ns)), h_lam=np.zeros((mi, nlam, ns)),
                        h_tcost=np.zeros((mi, nlam, ns)), h_tprior=np.zeros((mi, nlam, ns)),
                        h_status=np.zeros((mi, nlam, ns), dtype=np.int32), h_best=np.zeros((mi, ns), dtype=np.int32),
                        h_accept=np.zeros((mi, ns), dtype=np.int32), h_work=np.zeros((mi, 2), dtype=np.int64))
        elif history:                                   # (a subset of the names: only the library can refuse it)
            hist = {name: np.zeros(1) for name in history}
        rin = RetrieveIn(int(max_iter), nlam, int(mode), _p(ff), lam0, lam_min, lam_max, tol,
                         None if pri[0] is None else _p(pri[0]), None if pri[1] is None else _p(pri[1]))
        rout = RetrieveOut()
        for name, ctype in RetrieveOut._fields_:
            arr = res.get(name, hist.get(name))
            if arr is not None:
                setattr(rout, name, arr.ctypes.data_as(ctype))
        ret = atm_ret
        if ret is None:
            ret = abi.atm_t()
            C.memmove(C.byref(ret), C.byref(atm), C.sizeof(abi.atm_t))
        garr = (dp * 7)(*[_p(g[i]) for i in range(7)])
        tarr = (dp * 3)(*[_p(tp[i]) for i in range(3)])
        try:
            _chk(lib().jur_retrieve_scene_host(self.h, C.byref(atm), C.byref(ret), nr, garr, _p(rad), _p(tau), tarr,
                                               npts.ctypes.data_as(C.POINTER(C.c_int)), rp.ctypes.data_as(C.POINTER(C.c_long)),
                                               _p(yy), _p(ww), C.byref(rin), C.byref(rout), max_rays_per_pass))
        except JurassicError as e:                      # (what the iterations that completed left in the per-slice arrays)
            e.partial = dict(res, **(hist if history is True else {}))
            raise
        out = dict(lay, atm=ret, rad=rad, tau=tau, tp=np.ascontiguousarray(tp.T), np=npts, **res)
        if history is True:
            out.update(hist)
        return out

    def solve_slices(self, wptr, A, b, lam, mode=0, prior_ivar=None, prior_dx=None, want_factor=False):
        """Batched Cholesky solve of damped, optionally regularised systems the caller holds (jur_solve_slices_host): the
        re-solve of a Levenberg-Marquardt iteration.  wptr (nslice + 1,): running sum of the widths; A flat, A_s at the
        running sum of the squared widths, [w][w] (diagonal and lower triangle are read); b (n,).  lam: a scalar, (nlam,)
        or (nlam, nslice).  mode: DAMP_MARQUARDT or DAMP_PRIOR; prior_ivar, prior_dx (n,): both or neither.
        -> dict(dx (nlam, n), pred (nlam, nslice), status (nlam, nslice)) and, with want_factor, L (nlam, A.size)."""
        wp = np.ascontiguousarray(wptr, dtype=np.int64)
        ns = len(wp) - 1
        n, na = int(wp[-1]), int((np.diff(wp) ** 2).sum())
        AA, bb = (np.ascontiguousarray(x, dtype=np.float64).ravel() for x in (A, b))
        if AA.size != na or bb.size != n:
            raise ValueError("A must hold %d doubles and b %d" % (na, n))
        sin, sout, res, keep = _solve_structs(ns, n, na, lam, mode, prior_ivar, prior_dx, want_factor)
        _chk(lib().jur_solve_slices_host(self.h, ns, wp.ctypes.data_as(C.POINTER(C.c_long)), _p(AA), _p(bb), C.byref(sin),
                                         C.byref(sout)))
        return res

    def diagnose_slices(self, wptr, A, prior_ivar=None, want_S=False, want_avk=False):
        """Posterior diagnostics of systems the caller holds (jur_diagnose_slices_host).  wptr, A: as solve_slices;
        prior_ivar (n,) or None: the inverse a-priori variances.  No damping: M = A + diag(prior_ivar).
        -> dict(sigma, sigma_noise, sigma_smooth, avk_diag (n,), dofs, status (nslice,)) and, where wanted, the flat S
        (posterior covariance) and avk (averaging kernel S A), laid out as A."""
        wp = np.ascontiguousarray(wptr, dtype=np.int64)
        ns = len(wp) - 1
        n, na = int(wp[-1]), int((np.diff(wp) ** 2).sum())
        AA = np.ascontiguousarray(A, dtype=np.float64).ravel()
        if AA.size != na:
            raise ValueError("A must hold %d doubles" % na)
        dout, res, keep = _diag_structs(ns, n, na, prior_ivar, want_S, want_avk)
        _chk(lib().jur_diagnose_slices_host(self.h, ns, wp.ctypes.data_as(C.POINTER(C.c_long)), _p(AA),
                                            None if keep is None else _p(keep), C.byref(dout)))
        return res

    def diagnose_scene(self, atm, geom, y, weight, prior_ivar=None, want_S=False, want_avk=False, want_normal=False,
                       want_k=False, rad_in=None, max_rays_per_pass=0, rowptr=None):
        """Posterior diagnostics of every slice of a scene (jur_diagnose_scene_host): normal_scene on atm followed by
        the diagnostics on the device; meant for the atm of retrieve_scene's result, with that call's prior_ivar.
        -> normal_scene's dict without A and b, plus diagnose_slices' dict laid out by scene_slices of these rays.
        want_normal: also A and b; want_k: also the blocks.  What is not wanted never leaves the device."""
        g, lay, rp, yy, ww, rad = self._scene_inputs(atm, geom, y, weight, rad_in, rowptr)
        nr, nd = g.shape[1], self.nd
        tau = np.zeros((nr, nd))
        tp = np.zeros((3, nr))
        npts = np.zeros(nr, dtype=np.int32)
        ns, n, na = len(lay["sfirst"]), int(lay["wptr"][-1]), int(lay["aptr"][-1])
        cost, nlive = np.zeros(ns), np.zeros(ns, dtype=np.int64)
        A, b = (np.zeros(na), np.zeros(n)) if want_normal else (None, None)
        k = np.zeros(int(lay["rowptr"][-1]) * nd) if want_k else None
        dout, res, keep = _diag_structs(ns, n, na, prior_ivar, want_S, want_avk)
        garr = (dp * 7)(*[_p(g[i]) for i in range(7)])
        tarr = (dp * 3)(*[_p(tp[i]) for i in range(3)])
        lp_ = C.POINTER(C.c_long)
        _chk(lib().jur_diagnose_scene_host(self.h, C.byref(atm), nr, garr, _p(rad), _p(tau), tarr,
                                           npts.ctypes.data_as(C.POINTER(C.c_int)), rp.ctypes.data_as(lp_), _p(yy), _p(ww),
                                           None if keep is None else _p(keep), C.byref(dout),
                                           _p(A) if want_normal else None, _p(b) if want_normal else None, _p(cost),
                                           nlive.ctypes.data_as(lp_), _p(k) if want_k else None, max_rays_per_pass))
        out = dict(lay, rad=rad, tau=tau, tp=np.ascontiguousarray(tp.T), np=npts, cost=cost, nlive=nlive, **res)
        if want_normal:
            out.update(A=A, b=b)
        if want_k:
            out["k"] = k
        return out

    def gain_slices(self, wptr, S, rowptr, sid, k, weight_eff, var=None, status=None, want_gain=True):
        """Gain matrix and error budget of systems and blocks the caller holds (jur_gain_slices_host).  wptr, S: as
        diagnose_slices' wptr and S; status (nslice,) its breakdowns or None; rowptr (nr + 1,), sid (nr,) and the flat k:
        the blocks as kernel_scene lays them out and the slice of every ray (-1: none); weight_eff (nr, nd): the effective
        weights, anything not > 0 is "not live"; var (ncomp, nr, nd) or None: the variances per error source.
        -> dict(gain: flat, laid out as k (with want_gain); sigma_comp (ncomp, n))."""
        wp = np.ascontiguousarray(wptr, dtype=np.int64)
        rp = np.ascontiguousarray(rowptr, dtype=np.int64)
        sd = np.ascontiguousarray(sid, dtype=np.int32)
        ns, nr, n, na = len(wp) - 1, len(rp) - 1, int(wp[-1]), int((np.diff(wp) ** 2).sum())
        ww = np.ascontiguousarray(weight_eff, dtype=np.float64)
        if ww.ndim != 2 or ww.shape[0] != nr or sd.shape != (nr,):
            raise ValueError("weight_eff must be (%d, nd) and sid (%d,)" % (nr, nr))
        nd = ww.shape[1]
        SS, kk = (np.ascontiguousarray(x, dtype=np.float64).ravel() for x in (S, k))
        if SS.size != na or kk.size != int(rp[-1]) * nd:
            raise ValueError("S must hold %d doubles and k %d" % (na, int(rp[-1]) * nd))
        st = None if status is None else np.ascontiguousarray(status, dtype=np.int32)
        if st is not None and st.shape != (ns,):
            raise ValueError("status must be (%d,)" % ns)
        gin, gout, res, keep = _gain_structs(n, nr, nd, int(rp[-1]) * nd, var, want_gain)
        ip_, lp_ = C.POINTER(C.c_int), C.POINTER(C.c_long)
        _chk(lib().jur_gain_slices_host(self.h, ns, wp.ctypes.data_as(lp_), _p(SS), None if st is None else st.ctypes.data_as(ip_),
                                        nr, nd, rp.ctypes.data_as(lp_), sd.ctypes.data_as(ip_), _p(kk), _p(ww), C.byref(gin),
                                        C.byref(gout)))
        return res

    def gain_scene(self, atm, geom, y, weight, var=None, prior_ivar=None, want_gain=False, want_S=False, want_avk=False,
                   want_normal=False, want_k=False, rad_in=None, max_rays_per_pass=0, rowptr=None):
        """diagnose_scene plus the gain matrix G = S K^T Se^-1 and the retrieval error per source (jur_gain_scene_host):
        var (ncomp, nr, nd) or None, the variances of up to 8 error sources (error_components makes upstream's two).
        -> diagnose_scene's dict, plus sigma_comp (ncomp, n) and, with want_gain, gain: flat, the block of ray r at
        rowptr[r] * nd as [nd][width], entry (id, i) the response of element i to measurement (r, id).  What is not
        wanted never leaves the device."""
        g, lay, rp, yy, ww, rad = self._scene_inputs(atm, geom, y, weight, rad_in, rowptr)
        nr, nd = g.shape[1], self.nd
        tau = np.zeros((nr, nd))
        tp = np.zeros((3, nr))
        npts = np.zeros(nr, dtype=np.int32)
        ns, n, na = len(lay["sfirst"]), int(lay["wptr"][-1]), int(lay["aptr"][-1])
        cost, nlive = np.zeros(ns), np.zeros(ns, dtype=np.int64)
        A, b = (np.zeros(na), np.zeros(n)) if want_normal else (None, None)
        nk = int(lay["rowptr"][-1]) * nd
        k = np.zeros(nk) if want_k else None
        dout, res, keep = _diag_structs(ns, n, na, prior_ivar, want_S, want_avk)
        gin, gout, gres, gkeep = _gain_structs(n, nr, nd, nk, var, want_gain)
        garr = (dp * 7)(*[_p(g[i]) for i in range(7)])
        tarr = (dp * 3)(*[_p(tp[i]) for i in range(3)])
        lp_ = C.POINTER(C.c_long)
        _chk(lib().jur_gain_scene_host(self.h, C.byref(atm), nr, garr, _p(rad), _p(tau), tarr,
                                       npts.ctypes.data_as(C.POINTER(C.c_int)), rp.ctypes.data_as(lp_), _p(yy), _p(ww),
                                       None if keep is None else _p(keep), C.byref(dout), C.byref(gin), C.byref(gout),
                                       _p(A) if want_normal else None, _p(b) if want_normal else None, _p(cost),
                                       nlive.ctypes.data_as(lp_), _p(k) if want_k else None, max_rays_per_pass))
        out = dict(lay, rad=rad, tau=tau, tp=np.ascontiguousarray(tp.T), np=npts, cost=cost, nlive=nlive, **res)
        out.update(gres)
        if want_normal:
            out.update(A=A, b=b)
        if want_k:
            out["k"] = k
        return out

    def param_slices(self, wptr, rowptr, rowptr_b, sid, gain, kb, weight_eff, var=None, cov=None, want_C=True):
        """Cross-state matrix and parameter-error budget of gains and parameter blocks the caller holds
        (jur_param_slices_host).  wptr, rowptr, sid, gain, weight_eff: what gain_slices takes and returns; kb, rowptr_b:
        the flat blocks and the rowptr of kernel_scene on the same rays under other retrieval windows; var (nvar, nbw) or
        None: diagonal parameter covariances, laid out by bwptr; cov (ncov, nbb) or None: full ones, Sigma_s flat at
        bbptr[s] as (wb_s, wb_s), its diagonal and lower triangle read.
        -> dict(C: flat, C_s at cptr[s] as (w_s, wb_s) (with want_C); sigma_param (nvar + ncov, n), the var components
        first; bwptr, cptr, bbptr of param_layout)."""
        wp = np.ascontiguousarray(wptr, dtype=np.int64)
        rp = np.ascontiguousarray(rowptr, dtype=np.int64)
        rb = np.ascontiguousarray(rowptr_b, dtype=np.int64)
        sd = np.ascontiguousarray(sid, dtype=np.int32)
        ns, nr, n = len(wp) - 1, len(rp) - 1, int(wp[-1])
        ww = np.ascontiguousarray(weight_eff, dtype=np.float64)
        if ww.ndim != 2 or ww.shape[0] != nr or sd.shape != (nr,) or rb.shape != rp.shape:
            raise ValueError("weight_eff must be (%d, nd), sid (%d,) and rowptr_b (%d,)" % (nr, nr, nr + 1))
        nd = ww.shape[1]
        lay = param_layout(wp, rp, rb, sd)
        gg, kk = (np.ascontiguousarray(x, dtype=np.float64).ravel() for x in (gain, kb))
        if gg.size != int(rp[-1]) * nd or kk.size != int(rb[-1]) * nd:
            raise ValueError("gain must hold %d doubles and kb %d" % (int(rp[-1]) * nd, int(rb[-1]) * nd))
        nbw, nbb, nc = int(lay["bwptr"][-1]), int(lay["bbptr"][-1]), int(lay["cptr"][-1])
        vv = None if var is None else np.ascontiguousarray(var, dtype=np.float64)
        cc = None if cov is None else np.ascontiguousarray(cov, dtype=np.float64)
        if vv is not None and (vv.ndim != 2 or vv.shape[1] != nbw):
            raise ValueError("var must be (nvar, %d)" % nbw)
        if cc is not None and (cc.ndim != 2 or cc.shape[1] != nbb):
            raise ValueError("cov must be (ncov, %d)" % nbb)
        nvar, ncov = 0 if vv is None else vv.shape[0], 0 if cc is None else cc.shape[0]
        res = dict(lay, sigma_param=np.zeros((nvar + ncov, n)))
        if want_C:
            res["C"] = np.zeros(nc)
        pin = ParamIn(nvar, ncov, _p(vv) if nvar else None, _p(cc) if ncov else None)
        pout = ParamOut(_p(res["C"]) if want_C else None, _p(res["sigma_param"]) if nvar + ncov else None)
        ip_, lp_ = C.POINTER(C.c_int), C.POINTER(C.c_long)
        _chk(lib().jur_param_slices_host(self.h, ns, wp.ctypes.data_as(lp_), lay["bwptr"].ctypes.data_as(lp_), nr, nd,
                                         rp.ctypes.data_as(lp_), rb.ctypes.data_as(lp_), sd.ctypes.data_as(ip_), _p(gg), _p(kk),
                                         _p(ww), C.byref(pin), C.byref(pout)))
        return res

    def param_scene(self, ctl_b, atm, geom, y, weight, var_b=None, cov_b=None, prior_ivar=None, rad_in=None, var=None,
                    want_gain=False, want_kb=False, want_C=True, max_rays_per_pass=0):
        """The error that quantities b which are not retrieved leave in the retrieved state of a scene, in one call
        (jur_param_scene_host): what param_error_scene computes, bit for bit, with the gain and the blocks K_b of the
        parameters left on the device.  ctl_b: its retrieval windows define the parameters; var_b (nvar, bwptr[-1]) /
        cov_b (ncov, bbptr[-1]) as for param_slices; var (ncomp, nr, nd) as for gain_scene.
        -> the dict of param_error_scene (gain only with want_gain, C only with want_C), plus kb with want_kb: the flat
        blocks of kernel_scene under ctl_b, laid out by rowptr_b."""
        g, lay, rp, yy, ww, rad = self._scene_inputs(atm, geom, y, weight, rad_in, None)
        nr, nd = g.shape[1], self.nd
        cb = abi.ctl_t()
        C.memmove(C.byref(cb), C.byref(self.ctl), C.sizeof(abi.ctl_t))
        for name in ("retp_zmin", "retp_zmax", "rett_zmin", "rett_zmax", "retq_zmin", "retq_zmax", "retk_zmin", "retk_zmax"):
            setattr(cb, name, getattr(ctl_b, name))
        rb = _scene_layout(cb, atm, g[0] if nr else np.zeros(0))["rowptr"]
        play = param_layout(lay["wptr"], rp, rb, lay["sid"])
        ns, n, na = len(lay["sfirst"]), int(lay["wptr"][-1]), int(lay["aptr"][-1])
        nbw, nbb, nc = int(play["bwptr"][-1]), int(play["bbptr"][-1]), int(play["cptr"][-1])
        vv = None if var_b is None else np.ascontiguousarray(var_b, dtype=np.float64)
        cc = None if cov_b is None else np.ascontiguousarray(cov_b, dtype=np.float64)
        if vv is not None and (vv.ndim != 2 or vv.shape[1] != nbw):
            raise ValueError("var_b must be (nvar, %d)" % nbw)
        if cc is not None and (cc.ndim != 2 or cc.shape[1] != nbb):
            raise ValueError("cov_b must be (ncov, %d)" % nbb)
        nvar, ncov = 0 if vv is None else vv.shape[0], 0 if cc is None else cc.shape[0]
        tau = np.zeros((nr, nd))
        tp = np.zeros((3, nr))
        npts = np.zeros(nr, dtype=np.int32)
        cost, nlive = np.zeros(ns), np.zeros(ns, dtype=np.int64)
        dout, res, keep = _diag_structs(ns, n, na, prior_ivar, False, False)
        gin, gout, gres, gkeep = _gain_structs(n, nr, nd, int(rp[-1]) * nd, var, want_gain)
        pres = dict(play, sigma_param=np.zeros((nvar + ncov, n)), rowptr_b=rb, weight_eff=np.zeros((nr, nd)))
        if want_C:
            pres["C"] = np.zeros(nc)
        if want_kb:
            pres["kb"] = np.zeros(int(rb[-1]) * nd)
        lp_ = C.POINTER(C.c_long)
        pin = ParamIn(nvar, ncov, _p(vv) if nvar else None, _p(cc) if ncov else None)
        pout = ParamOut(_p(pres["C"]) if want_C else None, _p(pres["sigma_param"]) if nvar + ncov else None)
        sin = ParamSceneIn(C.addressof(ctl_b), rb.ctypes.data_as(lp_), play["bwptr"].ctypes.data_as(lp_), C.pointer(pin))
        sout = ParamSceneOut(C.pointer(pout), _p(pres["kb"]) if want_kb else None, _p(pres["weight_eff"]))
        garr = (dp * 7)(*[_p(g[i]) for i in range(7)])
        tarr = (dp * 3)(*[_p(tp[i]) for i in range(3)])
        _chk(lib().jur_param_scene_host(self.h, C.byref(atm), nr, garr, _p(rad), _p(tau), tarr,
                                        npts.ctypes.data_as(C.POINTER(C.c_int)), rp.ctypes.data_as(lp_), _p(yy), _p(ww),
                                        None if keep is None else _p(keep), C.byref(dout), C.byref(gin), C.byref(gout),
                                        C.byref(sin), C.byref(sout), None, None, _p(cost), nlive.ctypes.data_as(lp_), None,
                                        max_rays_per_pass))
        out = dict(lay, rad=rad, tau=tau, tp=np.ascontiguousarray(tp.T), np=npts, cost=cost, nlive=nlive, **res)
        out.update(gres)
        out.update(pres)
        out["elements_b"] = [scene_elements(ctl_b, atm, int(f), int(l)) for f, l in zip(out["sfirst"], out["slen"])]
        return out

    def cross_ms(self):
        """The share of param_scene's per-pass kernel within scene_ms (call kernel_ms first)."""
        ms, n = C.c_double(0), C.c_long(0)
        _chk(lib().jur_model_last_cross_ms(self.h, C.byref(ms), C.byref(n)))
        return dict(cross_ms=ms.value, cross_launches=n.value)

    def scene_bytes(self):
        """The device bytes the scene entries hold at present: their slab and param_scene's buffer beside it."""
        return lib().jur_model_scene_bytes(self.h)

    def set_ret_windows(self, ctl):
        """The retrieval windows of ctl (retp, rett, retq[ng], retk[nw] _zmin/_zmax, nothing else) become the model's
        (jur_model_set_ret_windows): from the next call on kernel_scene and the other scene entries, kernel and
        state_size derive their state from them.  No device work.  The layouts made on the Python side follow: the Model
        then holds a ctl_t of its own, the one it was created with plus these windows."""
        _chk(lib().jur_model_set_ret_windows(self.h, C.byref(ctl)))
        self.ctl = self.ret_windows(base=self.ctl)

    def ret_windows(self, base=None):
        """The retrieval windows that are set (jur_model_ret_windows) -> a new ctl_t: a copy of base (default: the ctl_t
        the Model lays its blocks out with) with the model's windows written into it."""
        out = abi.ctl_t()
        C.memmove(C.byref(out), C.byref(self.ctl if base is None else base), C.sizeof(abi.ctl_t))
        _chk(lib().jur_model_ret_windows(self.h, C.byref(out)))
        return out

    def scene_ms(self):
        """The share of kernel_scene's own kernels in the launches timed since the last call (call kernel_ms first)."""
        ms, n = C.c_double(0), C.c_long(0)
        _chk(lib().jur_model_last_scene_ms(self.h, C.byref(ms), C.byref(n)))
        return dict(scene_ms=ms.value, scene_launches=n.value)

    # known-answer hooks: device functions on arrays (include/jurassic_hip.h)
    def kat_ega_eps(self, ig, id_, tau, t, u, p, mode=3, chain=False):
        a = [np.ascontiguousarray(x, dtype=np.float64) for x in (tau, t, u, p)]
        out = np.zeros(len(a[0]))
        _chk(lib().jur_kat_ega_eps(self.h, ig, id_, len(out), *[_p(x) for x in a], mode, int(chain), _p(out)))
        return out

    def kat_cga_eps(self, ig, id_, tau, cgt, cgu, cgp, mode=3, chain=False):
        """Curtis-Godson look-up (FORMOD 1): the new path transmittance from tau and the means -> [n]"""
        a = [np.ascontiguousarray(x, dtype=np.float64) for x in (tau, cgt, cgu, cgp)]
        out = np.zeros(len(a[0]))
        _chk(lib().jur_kat_cga_eps(self.h, ig, id_, len(out), *[_p(x) for x in a], mode, int(chain), _p(out)))
        return out

    def kat_continua(self, id_, p, t, q, u_co2, u_h2o):
        a = [np.ascontiguousarray(x, dtype=np.float64) for x in (p, t, q, u_co2, u_h2o)]
        out = np.zeros((4, len(a[0])))
        _chk(lib().jur_kat_continua(self.h, id_, out.shape[1], *[_p(x) for x in a], _p(out)))
        return out

    def kat_update(self, id_, what, a, b, c, rad, tau):
        """what 0: one segment (a = T, b = tau_gas, c = beta_ds); what 1: epilogue (a = tsurf, b = bbt flag).
        -> (rad, tau, src)"""
        a, b, c = (np.ascontiguousarray(x, dtype=np.float64) for x in (a, b, c))
        rad, tau = np.array(rad, dtype=np.float64), np.array(tau, dtype=np.float64)
        src = np.zeros(len(a))
        _chk(lib().jur_kat_update(self.h, id_, len(a), what, _p(a), _p(b), _p(c), _p(rad), _p(tau), _p(src)))
        return rad, tau, src

    def kat_traceray(self, geom, overflow_ok=False):
        """The batched ray tracer's LOS records (jur_kat_traceray).  geom: (nr, 7) -> dict(p, t, ds, qh2o (nr, NLOS),
        k (nw, nr, NLOS), u (ng, nr, NLOS), np, tsurf (nr,), tp (nr, 3), status); entries from np[ray] on are 0.
        overflow_ok: a ray that needs NLOS points comes back clamped with status == ENLOS instead of raising."""
        g = np.ascontiguousarray(np.asarray(geom, dtype=np.float64).T)
        nr = g.shape[1]
        nw = self.nw
        los = np.zeros((nr, 4 + nw + self.ng, abi.NLOS))
        tsurf = np.zeros(nr)
        tp = np.zeros((3, nr))
        npts = np.zeros(nr, dtype=np.int32)
        garr = (dp * 7)(*[_p(g[k]) for k in range(7)])
        tarr = (dp * 3)(*[_p(tp[k]) for k in range(3)])
        rc = lib().jur_kat_traceray(self.h, nr, garr, _p(los), _p(tsurf), tarr, npts.ctypes.data_as(C.POINTER(C.c_int)))
        if not (overflow_ok and rc == ENLOS):
            _chk(rc)
        return dict(p=los[:, 0], t=los[:, 1], ds=los[:, 2], qh2o=los[:, 3],
                    k=np.ascontiguousarray(los[:, 4:4 + nw].transpose(1, 0, 2)),
                    u=np.ascontiguousarray(los[:, 4 + nw:].transpose(1, 0, 2)),
                    np=npts, tsurf=tsurf, tp=np.ascontiguousarray(tp.T), status=rc)

    def kat_cloud_mean(self, a0, length, z0, lat0, x0):
        """Rule 4 of IP 3 on the device (jur_kat_cloud_mean) over the atmosphere points [a0, a0 + length) at the
        positions z0, lat0 (n,), x0 (n, 3) = geo2cart(0, lon0, lat0) -> (2 + ng + nw, n): p, T, q, k."""
        z0, lat0, x0 = (np.ascontiguousarray(x, dtype=np.float64) for x in (z0, lat0, x0))
        n = len(z0)
        if lat0.shape != (n,) or x0.shape != (n, 3):
            raise ValueError("kat_cloud_mean: z0, lat0 (n,) and x0 (n, 3)")
        out = np.zeros((2 + self.ng + max(self.nw, 1), n))
        _chk(lib().jur_kat_cloud_mean(self.h, n, int(a0), int(length), _p(z0), _p(lat0), _p(x0), _p(out)))
        return out

    def enable_timing(self, on=True):
        _chk(lib().jur_model_enable_timing(self.h, int(on)))

    def kernel_ms(self):
        ms = (C.c_double * 3)()
        n = (C.c_long * 3)()
        _chk(lib().jur_model_last_kernel_ms(self.h, ms, n))
        pm, pn = C.c_double(0), C.c_long(0)
        _chk(lib().jur_model_last_pencil_ms(self.h, C.byref(pm), C.byref(pn)))
        return dict(trace_ms=ms[0], ega_ms=ms[1], combine_ms=ms[2], trace_launches=n[0], ega_launches=n[1],
                    combine_launches=n[2], pencil_ms=pm.value, pencil_launches=pn.value)

    def contrib_ms(self):
        """The contribution kernel's share of the launches timed since the last call (call kernel_ms first)."""
        ms, n = C.c_double(0), C.c_long(0)
        _chk(lib().jur_model_last_contrib_ms(self.h, C.byref(ms), C.byref(n)))
        return dict(contrib_ms=ms.value, contrib_launches=n.value)

    def workspace_bytes(self):
        return lib().jur_model_workspace_bytes(self.h)

    def last_launches(self):
        """Integration launches of the last batched call."""
        return lib().jur_model_last_launches(self.h)

    def set_compact_workspace(self, on):
        _chk(lib().jur_model_set_compact_workspace(self.h, int(on)))

    def table_bytes(self):
        return lib().jur_model_table_bytes(self.h)


ARITH_FAST, ARITH_EXACT = 0, 1
DAMP_MARQUARDT, DAMP_PRIOR = 0, 1      # JUR_DAMP_MARQUARDT, JUR_DAMP_PRIOR
EINVAL = -1                            # JUR_EINVAL
ENLOS = -5                             # JUR_ENLOS


class SolveIn(C.Structure):
    """jur_solve_in_t"""
    _fields_ = [("nlam", C.c_int), ("mode", C.c_int), ("lam", dp), ("prior_ivar", dp), ("prior_dx", dp)]


class SolveOut(C.Structure):
    """jur_solve_out_t"""
    _fields_ = [("dx", dp), ("pred", dp), ("status", C.POINTER(C.c_int)), ("L", dp)]


class DiagOut(C.Structure):
    """jur_diag_out_t"""
    _fields_ = [("sigma", dp), ("sigma_noise", dp), ("sigma_smooth", dp), ("avk_diag", dp), ("dofs", dp),
                ("status", C.POINTER(C.c_int)), ("S", dp), ("avk", dp)]


class GainIn(C.Structure):
    """jur_gain_in_t"""
    _fields_ = [("ncomp", C.c_int), ("var", dp)]


class GainOut(C.Structure):
    """jur_gain_out_t"""
    _fields_ = [("gain", dp), ("sigma_comp", dp)]


class ParamIn(C.Structure):
    """jur_param_in_t"""
    _fields_ = [("nvar", C.c_int), ("ncov", C.c_int), ("var", dp), ("cov", dp)]


class ParamOut(C.Structure):
    """jur_param_out_t"""
    _fields_ = [("C", dp), ("sigma_param", dp)]


class ParamSceneIn(C.Structure):
    """jur_param_scene_in_t"""
    _fields_ = [("ctl_b", C.c_void_p), ("rowptr_b", C.POINTER(C.c_long)), ("bwptr", C.POINTER(C.c_long)),
                ("in_", C.POINTER(ParamIn))]


class ParamSceneOut(C.Structure):
    """jur_param_scene_out_t"""
    _fields_ = [("out", C.POINTER(ParamOut)), ("kb", dp), ("weight_eff", dp)]


RET_ACTIVE, RET_CONVERGED, RET_STALLED, RET_MAXITER = 0, 1, 2, 3      # JUR_RET_*
RET_FAILED = 4                         # JUR_RET_FAILED: the slice's current state could not be traced (OVERFLOW_ISOLATE)
OVERFLOW_ERROR, OVERFLOW_ISOLATE = 0, 1                               # JUR_OVERFLOW_*
TRIAL_OVERFLOW = -2                    # JUR_TRIAL_OVERFLOW, a value of h_status: a ray of that trial could not be traced


def np_overflows(npts):
    """jur_np_overflows (host arithmetic, no GPU): does a ray with that many LOS points count as untraceable?"""
    return bool(lib().jur_np_overflows(int(npts)))


class RetrieveIn(C.Structure):
    """jur_retrieve_in_t"""
    _fields_ = [("max_iter", C.c_int), ("nlam", C.c_int), ("mode", C.c_int), ("fac", dp), ("lam0", C.c_double),
                ("lam_min", C.c_double), ("lam_max", C.c_double), ("tol", C.c_double), ("prior_ivar", dp), ("prior_xa", dp)]


_ip, _lp = C.POINTER(C.c_int), C.POINTER(C.c_long)


class RetrieveOut(C.Structure):
    """jur_retrieve_out_t"""
    _fields_ = [("x", dp), ("lam", dp), ("cost", dp), ("prior", dp), ("nlive", _lp), ("state", _ip), ("iters", _ip),
                ("h_cost", dp), ("h_prior", dp), ("h_lam", dp), ("h_tcost", dp), ("h_tprior", dp), ("h_status", _ip),
                ("h_best", _ip), ("h_accept", _ip), ("h_work", _lp)]


def retrieve_decide(J, Jt, lamt, status, lam, state, tol, lam_max, fac_max):
    """jur_retrieve_decide (host arithmetic, no GPU): the accept/reject policy of one iteration of Model.retrieve_scene.
    J (nslice,); Jt, lamt, status (nlam, nslice); lam, state (nslice,) -> dict(lam, state: the updated copies; best,
    accept: -1 for a slice that is not RET_ACTIVE)."""
    JJ = np.ascontiguousarray(J, dtype=np.float64)
    ns = len(JJ)
    T, LT = (np.ascontiguousarray(x, dtype=np.float64).reshape(-1, ns) for x in (Jt, lamt))
    S = np.ascontiguousarray(status, dtype=np.int32).reshape(-1, ns)
    nlam = T.shape[0]
    if LT.shape != T.shape or S.shape != T.shape:
        raise ValueError("Jt, lamt and status must be (nlam, %d)" % ns)
    lm = np.array(lam, dtype=np.float64)
    st = np.array(state, dtype=np.int32)
    if lm.shape != (ns,) or st.shape != (ns,):
        raise ValueError("lam and state must be (%d,)" % ns)
    best, accept = np.zeros(ns, dtype=np.int32), np.zeros(ns, dtype=np.int32)
    ip_ = C.POINTER(C.c_int)
    _chk(lib().jur_retrieve_decide(nlam, ns, tol, lam_max, fac_max, _p(JJ), _p(T), _p(LT), S.ctypes.data_as(ip_), _p(lm),
                                   st.ctypes.data_as(ip_), best.ctypes.data_as(ip_), accept.ctypes.data_as(ip_)))
    return dict(lam=lm, state=st, best=best, accept=accept)


def state_bounds_upstream(ctl):
    """jur_state_bounds_upstream: (lo, hi) of upstream's box for the control's quantities -- p in [5e-7, 5e4], T in
    [100, 400], q in [0, 1], k in [0, +inf]."""
    nq = _chk(lib().jur_state_bounds_upstream(C.byref(ctl), None, None))
    lo, hi = np.zeros(nq), np.zeros(nq)
    _chk(lib().jur_state_bounds_upstream(C.byref(ctl), _p(lo), _p(hi)))
    return lo, hi


def state_bound(x, lo, hi):
    """jur_state_bound on scalars or arrays (broadcast): the library's own arithmetic, element by element."""
    xs, ls, hs = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64))
    f = lib().jur_state_bound
    out = np.array([f(float(a), float(b), float(c)) for a, b, c in zip(xs.ravel(), ls.ravel(), hs.ravel())], dtype=np.float64).reshape(xs.shape)
    return out if out.ndim else float(out)


def state_on_bounds(lo, hi, iq, x):
    """jur_state_on_bounds: side (int8, -1 / 0 / +1 per element: at its lower bound, at neither, at its upper bound) for
    the elements x of the quantities iq under the box (lo, hi) per quantity, and their number -> dict(side, count)."""
    l, h = (np.ascontiguousarray(v, dtype=np.float64).ravel() for v in (lo, hi))
    if len(l) != len(h):
        raise ValueError("lo and hi must have one entry per quantity each")
    q = np.ascontiguousarray(iq, dtype=np.int32).ravel()
    xs = np.ascontiguousarray(x, dtype=np.float64).ravel()
    if len(q) != len(xs):
        raise ValueError("iq and x must have one entry per element each")
    side = np.zeros(len(xs), dtype=np.int8)
    n = _chk(lib().jur_state_on_bounds(len(l), _p(l), _p(h), len(xs), q.ctypes.data_as(C.POINTER(C.c_int)), _p(xs),
                                       side.ctypes.data_as(C.POINTER(C.c_byte))))
    return dict(side=side, count=int(n))


def _solve_structs(ns, n, na, lam, mode, prior_ivar, prior_dx, want_factor):
    """(jur_solve_in_t, jur_solve_out_t, the result dict, the input arrays to keep alive) of ns systems with n elements
    and na matrix entries in all.  Nothing is refused here that the library refuses."""
    lm = np.asarray(lam, dtype=np.float64)
    if lm.ndim == 0:
        lm = lm.reshape(1, 1)
    elif lm.ndim == 1:
        lm = lm.reshape(-1, 1)
    if lm.ndim != 2 or lm.shape[1] not in (1, ns):
        raise ValueError("lam must be a scalar, (nlam,) or (nlam, %d)" % ns)
    nlam = lm.shape[0]
    lm = np.ascontiguousarray(np.broadcast_to(lm, (nlam, ns)))
    pri = [None if x is None else np.ascontiguousarray(x, dtype=np.float64).ravel() for x in (prior_ivar, prior_dx)]
    if any(x is not None and x.size != n for x in pri):
        raise ValueError("prior_ivar and prior_dx must hold %d doubles" % n)
    res = dict(dx=np.zeros((nlam, n)), pred=np.zeros((nlam, ns)), status=np.zeros((nlam, ns), dtype=np.int32))
    if want_factor:
        res["L"] = np.zeros((nlam, na))
    sin = SolveIn(nlam, int(mode), _p(lm), None if pri[0] is None else _p(pri[0]), None if pri[1] is None else _p(pri[1]))
    sout = SolveOut(_p(res["dx"]), _p(res["pred"]), res["status"].ctypes.data_as(C.POINTER(C.c_int)),
                    _p(res["L"]) if want_factor else None)
    return sin, sout, res, (lm, pri)


def _diag_structs(ns, n, na, prior_ivar, want_S, want_avk):
    """(jur_diag_out_t, the result dict, prior_ivar as the array to keep alive or None) of ns systems with n elements
    and na matrix entries in all.  Nothing is refused here that the library refuses."""
    pri = None if prior_ivar is None else np.ascontiguousarray(prior_ivar, dtype=np.float64).ravel()
    if pri is not None and pri.size != n:
        raise ValueError("prior_ivar must hold %d doubles" % n)
    res = dict(sigma=np.zeros(n), sigma_noise=np.zeros(n), sigma_smooth=np.zeros(n), avk_diag=np.zeros(n),
               dofs=np.zeros(ns), status=np.zeros(ns, dtype=np.int32))
    if want_S:
        res["S"] = np.zeros(na)
    if want_avk:
        res["avk"] = np.zeros(na)
    dout = DiagOut(_p(res["sigma"]), _p(res["sigma_noise"]), _p(res["sigma_smooth"]), _p(res["avk_diag"]), _p(res["dofs"]),
                   res["status"].ctypes.data_as(C.POINTER(C.c_int)), _p(res["S"]) if want_S else None,
                   _p(res["avk"]) if want_avk else None)
    return dout, res, pri


def _gain_structs(n, nr, nd, nk, var, want_gain):
    """(jur_gain_in_t, jur_gain_out_t, the result dict, var as the array to keep alive or None) of a call with n state
    elements, nr rays of nd channels and nk block doubles.  Nothing is refused here that the library refuses."""
    vv = None if var is None else np.ascontiguousarray(var, dtype=np.float64)
    if vv is not None and (vv.ndim != 3 or vv.shape[1:] != (nr, nd)):
        raise ValueError("var must be (ncomp, %d, %d)" % (nr, nd))
    ncomp = 0 if vv is None else vv.shape[0]
    res = dict(sigma_comp=np.zeros((ncomp, n)))
    if want_gain:
        res["gain"] = np.zeros(nk)
    gin = GainIn(ncomp, None if vv is None else _p(vv))
    gout = GainOut(_p(res["gain"]) if want_gain else None, _p(res["sigma_comp"]) if ncomp else None)
    return gin, gout, res, vv


def error_components(y, err_noise, err_formod):
    """jur_error_components (host arithmetic, no GPU; upstream's set_cov_meas): y (nr, nd) radiances, err_noise (nd,) in
    radiance units, err_formod (nd,) in per cent of the radiance -> (var (2, nr, nd): noise, forward model; weight (nr,
    nd) = 1 / their sum, 0 with both variances +0.0 where that sum is not finite and > 0)."""
    yy = np.ascontiguousarray(y, dtype=np.float64)
    if yy.ndim != 2:
        raise ValueError("y must be (nr, nd)")
    nr, nd = yy.shape
    en, ef = (np.ascontiguousarray(x, dtype=np.float64).ravel() for x in (err_noise, err_formod))
    if en.size != nd or ef.size != nd:
        raise ValueError("err_noise and err_formod must hold %d doubles" % nd)
    var, weight = np.zeros((2, nr, nd)), np.zeros((nr, nd))
    _chk(lib().jur_error_components(nd, nr, _p(yy), _p(en), _p(ef), _p(var), _p(weight)))
    return var, weight


def param_layout(wptr, rowptr, rowptr_b, sid):
    """jur_param_layout (host arithmetic, no GPU): the layout of param_slices' arrays.  wptr (nslice + 1,), rowptr (nr + 1,)
    and sid (nr,) of the retrieved state, rowptr_b (nr + 1,) of the parameter blocks on the same rays -> dict(bwptr, cptr,
    bbptr (nslice + 1,)): the running sums of wb_s, the width in rowptr_b of the rays of slice s (0 without rays), of
    w_s * wb_s and of wb_s^2.  Raises JurassicError where the widths do not fit together."""
    wp, rp, rb = (np.ascontiguousarray(x, dtype=np.int64).ravel() for x in (wptr, rowptr, rowptr_b))
    sd = np.ascontiguousarray(sid, dtype=np.int32).ravel()
    ns, nr = len(wp) - 1, len(rp) - 1
    if ns < 0 or nr < 0 or len(rb) != nr + 1 or len(sd) != nr:
        raise ValueError("rowptr and rowptr_b must hold one entry more than sid, and wptr one at least")
    ip_, lp_ = C.POINTER(C.c_int), C.POINTER(C.c_long)
    bw, cp, bb = (np.zeros(ns + 1, dtype=np.int64) for _ in range(3))
    _chk(lib().jur_param_layout(ns, wp.ctypes.data_as(lp_), nr, rp.ctypes.data_as(lp_), rb.ctypes.data_as(lp_),
                                sd.ctypes.data_as(ip_), bw.ctypes.data_as(lp_), cp.ctypes.data_as(lp_), bb.ctypes.data_as(lp_)))
    return dict(bwptr=bw, cptr=cp, bbptr=bb)


def param_error_scene(model, ctl_b, atm, geom, y, weight, var_b=None, cov_b=None, prior_ivar=None, rad_in=None,
                      max_rays_per_pass=0):
    """The error that quantities b which are not retrieved leave in the retrieved state of a scene, with one model:
    gain_scene(want_gain=True) under the model's own retrieval windows, the effective weights by that entry's liveness
    rule (with a field of view set: scene_fov_live), kernel_scene under the windows of ctl_b for K_b -- the model's own
    are put back afterwards, after an error too -- and param_slices.  var_b (nvar, bwptr[-1]) / cov_b (ncov, bbptr[-1]):
    the covariances of b, laid out over elements_b; prior_corr_slices(model, bwptr, iq, z, sigma, cz, want_Sa=True)["Sa"]
    is one cov_b row.
    -> gain_scene's dict (with gain), plus C, cptr, bwptr, bbptr, sigma_param of param_slices, rowptr_b, weight_eff and
    elements_b: per slice scene_elements(ctl_b, atm, sfirst[s], slen[s]), the parameters the columns of C_s stand for."""
    out = model.gain_scene(atm, geom, y, weight, prior_ivar=prior_ivar, want_gain=True, rad_in=rad_in,
                           max_rays_per_pass=max_rays_per_pass)
    g = np.asarray(geom, dtype=np.float64)
    yy, ww = (np.asarray(x, dtype=np.float64) for x in (y, weight))
    if rad_in is None:
        seen = np.ones(yy.shape, dtype=bool)
    elif model.fov() is not None:
        seen = scene_fov_live(g[:, 0], rad_in)
    else:
        seen = np.isfinite(np.asarray(rad_in, dtype=np.float64))
    live = seen & np.isfinite(out["rad"]) & np.isfinite(yy) & (ww > 0) & (out["sid"] >= 0)[:, None]
    weff = np.where(live, ww, 0.0)
    own = model.ret_windows()
    model.set_ret_windows(ctl_b)
    try:
        kb = model.kernel_scene(atm, geom, rad_in=rad_in, max_rays_per_pass=max_rays_per_pass)
    finally:
        model.set_ret_windows(own)
    res = model.param_slices(out["wptr"], out["rowptr"], kb["rowptr"], out["sid"], out["gain"], kb["k"], weff, var=var_b,
                             cov=cov_b)
    out.update(res)
    out.update(rowptr_b=kb["rowptr"], weight_eff=weff,
               elements_b=[scene_elements(ctl_b, atm, int(f), int(l)) for f, l in zip(out["sfirst"], out["slen"])])
    return out


def avk_summary(ctl, atm, first, length, avk):
    """jur_avk_summary (host arithmetic, no GPU): what is read off the averaging kernel avk (w, w) of the slice
    [first, first + length) -> dict(dofs_q (2 + ng + nw,): the trace per quantity; area (w,): the row sums within the
    element's quantity; resolution (w,): dz / AVK_ii, +inf where AVK_ii is not > 0; iq, ip: scene_elements')."""
    el = scene_elements(ctl, atm, first, length)
    w = len(el["iq"])
    K = np.ascontiguousarray(avk, dtype=np.float64)
    if K.size != w * w:
        raise ValueError("avk must be (%d, %d)" % (w, w))
    dofs_q, area, res = np.zeros(2 + ctl.ng + ctl.nw), np.zeros(w), np.zeros(w)
    _chk(lib().jur_avk_summary(C.byref(ctl), C.byref(atm), int(first), int(length), _p(K), _p(dofs_q), _p(area), _p(res)))
    return dict(dofs_q=dofs_q, area=area, resolution=res, iq=el["iq"], ip=el["ip"])


def solve_slices(model, wptr, A, b, lam, **kw):
    """Model.solve_slices as a function"""
    return model.solve_slices(wptr, A, b, lam, **kw)


class GslMatrix(C.Structure):
    """Layout of GSL's gsl_matrix (jur_gsl_matrix_t): what the reference's kernel() takes."""
    _fields_ = [("size1", C.c_size_t), ("size2", C.c_size_t), ("tda", C.c_size_t), ("data", dp), ("block", C.c_void_p),
                ("owner", C.c_int)]


def kernel(ctl, atm, obs, m, n, tda=None):
    """Drop-in kernel() (reference jurassic.c:812): -> (m, n) Jacobian; obs receives the unperturbed forward model.
    tda > n exercises a matrix whose rows are longer than its width (a sub-matrix view)."""
    tda = tda or n
    store = np.full((m, tda), -7.0)
    mat = GslMatrix(m, n, tda, _p(store), None, 0)
    lib().kernel(C.byref(ctl), C.byref(atm), C.byref(obs), C.byref(mat))
    assert np.all(store[:, n:] == -7.0)               # nothing written beyond the matrix's width
    return store[:, :n].copy()


def _scene_layout(ctl, atm, time):
    t = np.ascontiguousarray(time, dtype=np.float64)
    nr = len(t)
    first, length = np.zeros(nr, dtype=np.int32), np.zeros(nr, dtype=np.int32)
    rowptr = np.zeros(nr + 1, dtype=np.int64)
    ip_ = C.POINTER(C.c_int)
    _chk(lib().jur_scene_layout(C.byref(ctl), C.byref(atm), nr, _p(t), first.ctypes.data_as(ip_), length.ctypes.data_as(ip_),
                                rowptr.ctypes.data_as(C.POINTER(C.c_long))))
    return dict(first=first, len=length, rowptr=rowptr)


def scene_layout(ctl, atm, time):
    """jur_scene_layout (host arithmetic, no GPU): the slice [first, first + len) of the atmosphere that every ray time
    stamp is traced through and the running sum rowptr (nr + 1,) of the block widths -> dict(first, len, rowptr)."""
    return _scene_layout(ctl, atm, time)


def scene_columns(ctl, atm, first, length):
    """jur_scene_columns: the global state indices (columns of Model.kernel's matrix) of the slice, ascending."""
    n = _chk(lib().jur_scene_columns(C.byref(ctl), C.byref(atm), int(first), int(length), None))
    cols = np.zeros(n, dtype=np.int64)
    _chk(lib().jur_scene_columns(C.byref(ctl), C.byref(atm), int(first), int(length), cols.ctypes.data_as(C.POINTER(C.c_long))))
    return cols


def scene_slices(ctl, atm, time):
    """jur_scene_slices (host arithmetic, no GPU): the distinct slices of width > 0 among the rays with these time
    stamps, in the order the rays first meet them -> dict(sid (nr,; -1: width 0), sfirst, slen (nslice,), wptr, aptr
    (nslice + 1,): running sums of the widths and of their squares)."""
    t = np.ascontiguousarray(time, dtype=np.float64)
    nr = len(t)
    ip_, lp_ = C.POINTER(C.c_int), C.POINTER(C.c_long)
    ns = _chk(lib().jur_scene_slices(C.byref(ctl), C.byref(atm), nr, _p(t), None, None, None, None, None))
    sid = np.zeros(nr, dtype=np.int32)
    sfirst, slen = np.zeros(ns, dtype=np.int32), np.zeros(ns, dtype=np.int32)
    wptr, aptr = np.zeros(ns + 1, dtype=np.int64), np.zeros(ns + 1, dtype=np.int64)
    _chk(lib().jur_scene_slices(C.byref(ctl), C.byref(atm), nr, _p(t), sid.ctypes.data_as(ip_), sfirst.ctypes.data_as(ip_),
                                slen.ctypes.data_as(ip_), wptr.ctypes.data_as(lp_), aptr.ctypes.data_as(lp_)))
    return dict(sid=sid, sfirst=sfirst, slen=slen, wptr=wptr, aptr=aptr)


def scene_ray_slices(ctl, atm, time):
    """jur_scene_ray_slices (host arithmetic, no GPU): the distinct slices of two points or more that rays with these time
    stamps are traced through, with or without state elements, in the order the rays first meet them
    -> dict(sfirst, slen)."""
    t = np.ascontiguousarray(time, dtype=np.float64).ravel()
    ip_ = C.POINTER(C.c_int)
    sfirst, slen = np.zeros(len(t), dtype=np.int32), np.zeros(len(t), dtype=np.int32)
    n = _chk(lib().jur_scene_ray_slices(C.byref(ctl), C.byref(atm), len(t), _p(t), sfirst.ctypes.data_as(ip_), slen.ctypes.data_as(ip_)))
    return dict(sfirst=sfirst[:n].copy(), slen=slen[:n].copy())


def scene_hydrostatic(ctl, hydz, atm, sfirst, slen):
    """jur_scene_hydrostatic (host arithmetic, no GPU): a new atm_t, atm with every segment [sfirst, sfirst + slen) of two
    points or more balanced on its own around the point nearest to hydz (upstream's hydrostatic_1d_h2o per profile)."""
    sf, sn = (np.ascontiguousarray(a, dtype=np.int32).ravel() for a in (sfirst, slen))
    if len(sf) != len(sn):
        raise ValueError("sfirst holds %d entries, slen %d" % (len(sf), len(sn)))
    ip_ = C.POINTER(C.c_int)
    out = abi.atm_t()
    C.memmove(C.byref(out), C.byref(atm), C.sizeof(abi.atm_t))
    _chk(lib().jur_scene_hydrostatic(C.byref(ctl), float(hydz), C.byref(atm), len(sf), sf.ctypes.data_as(ip_),
                                     sn.ctypes.data_as(ip_), C.byref(out)))
    return out


def scene_elements(ctl, atm, first, length):
    """jur_scene_elements: scene_columns plus the quantity (0 p, 1 T, 2 + g q, 2 + ng + w k) and the atmosphere point
    of every state element of the slice -> dict(cols, iq, ip)."""
    n = _chk(lib().jur_scene_elements(C.byref(ctl), C.byref(atm), int(first), int(length), None, None, None))
    cols, iq, ip = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    ip_ = C.POINTER(C.c_int)
    _chk(lib().jur_scene_elements(C.byref(ctl), C.byref(atm), int(first), int(length), cols.ctypes.data_as(C.POINTER(C.c_long)),
                                  iq.ctypes.data_as(ip_), ip.ctypes.data_as(ip_)))
    return dict(cols=cols, iq=iq, ip=ip)


def prior_corr_slices(model, wptr, iq, z, sigma, cz, want_Sa=True):
    """jur_prior_corr_host on systems the caller lays out: iq, z, sigma (n,) per element, cz (nq,) the correlation length
    of every quantity (0: uncorrelated) -> dict(R, Sa (flat, laid out as A), status (nslice,), wptr, aptr).  Sa_ij =
    sigma_i sigma_j exp(-|z_i - z_j| / cz[q]) within a quantity, R = Sa^-1 per slice, both formed on the device."""
    wp = np.ascontiguousarray(wptr, dtype=np.int64).ravel()
    ns, n = len(wp) - 1, int(wp[-1])
    ap = np.concatenate(([0], np.cumsum(np.diff(wp) ** 2))).astype(np.int64)
    qq = np.ascontiguousarray(iq, dtype=np.int32).ravel()
    zz, ss = (np.ascontiguousarray(x, dtype=np.float64).ravel() for x in (z, sigma))
    cc = np.ascontiguousarray(cz, dtype=np.float64).ravel()
    if qq.size != n or zz.size != n or ss.size != n:
        raise ValueError("iq, z and sigma must hold %d entries" % n)
    R, Sa = np.zeros(int(ap[-1])), np.zeros(int(ap[-1]) if want_Sa else 0)
    status = np.zeros(ns, dtype=np.int32)
    ip_ = C.POINTER(C.c_int)
    _chk(lib().jur_prior_corr_host(model.h, ns, wp.ctypes.data_as(C.POINTER(C.c_long)), qq.ctypes.data_as(ip_), _p(zz), _p(ss),
                                   len(cc), _p(cc), _p(R), _p(Sa) if want_Sa else None, status.ctypes.data_as(ip_)))
    return dict(R=R, Sa=Sa if want_Sa else None, status=status, wptr=wp, aptr=ap)


def prior_corr(model, ctl, atm, time, sigma_q, cz_q):
    """The upstream parametrisation of the a-priori covariance for the slices of a scene (jur_prior_corr_host): sigma_q
    and cz_q (2 + ng + nw,) give every quantity (0 p, 1 T, 2 + g q, 2 + ng + w k) its standard deviation and its vertical
    correlation length (0: uncorrelated); the altitudes are atm.z of the elements' points.  A sigma_q entry may be a
    callable of (values of the quantity at the elements' points) for a relative error.  -> dict(R, Sa, status, wptr, aptr,
    iq, ip, z, sigma), laid out by scene_slices of these time stamps: R goes to Model.set_prior_precision."""
    sl = scene_slices(ctl, atm, time)
    iq, ip = [], []
    for f, l in zip(sl["sfirst"], sl["slen"]):
        el = scene_elements(ctl, atm, int(f), int(l))
        iq.append(el["iq"]); ip.append(el["ip"])
    iq = np.concatenate(iq) if iq else np.zeros(0, dtype=np.int32)
    ip = np.concatenate(ip) if ip else np.zeros(0, dtype=np.int32)
    ng = ctl.ng
    sigma = np.zeros(len(iq))
    for e, (q, i) in enumerate(zip(iq, ip)):
        sq = sigma_q[q]
        if callable(sq):
            val = atm.p[i] if q == 0 else atm.t[i] if q == 1 else atm.q[q - 2][i] if q < 2 + ng else atm.k[q - 2 - ng][i]
            sq = sq(val)
        sigma[e] = sq
    z = np.array([atm.z[i] for i in ip], dtype=np.float64)
    out = prior_corr_slices(model, sl["wptr"], iq, z, sigma, cz_q)
    out.update(aptr=sl["aptr"], iq=iq, ip=ip, z=z, sigma=sigma)
    return out


def scene_blocks_to_dense(ctl, atm, out, n=None):
    """Scatters the blocks of Model.kernel_scene's result into the dense (nr * nd, n) matrix (row ray * nd + channel,
    the state's n columns; zero outside the blocks): for tests and small cases."""
    nr = len(out["first"])
    nd = out["rad"].shape[1]
    if n is None:
        n = len(scene_columns(ctl, atm, 0, atm.np))
    dense = np.zeros((nr * nd, n))
    rp, cache = out["rowptr"], {}
    for r in range(nr):
        w = int(rp[r + 1] - rp[r])
        if w == 0:
            continue
        key = (int(out["first"][r]), int(out["len"][r]))
        if key not in cache:
            cache[key] = scene_columns(ctl, atm, *key)
        dense[r * nd:(r + 1) * nd, cache[key]] = out["k"][rp[r] * nd:rp[r + 1] * nd].reshape(nd, w)
    return dense


def device_info(device):
    """-> dict(pci_bus_id, free, total) of a HIP device (jur_device_info)."""
    buf = C.create_string_buffer(64)
    f, t = C.c_size_t(0), C.c_size_t(0)
    _chk(lib().jur_device_info(device, buf, 64, C.byref(f), C.byref(t)))
    return dict(pci_bus_id=buf.value.decode(), free=int(f.value), total=int(t.value))


def _handles(models):
    return (C.c_void_p * len(models))(*[m.h for m in models])


def multi_balance(model, geom, nparts):
    """Boundaries of nparts contiguous ray ranges with equal estimated LOS points (jur_multi_balance)."""
    g = np.ascontiguousarray(np.asarray(geom, dtype=np.float64).T)
    garr = (dp * 7)(*[_p(g[k]) for k in range(7)])
    b = (C.c_long * (nparts + 1))()
    _chk(lib().jur_multi_balance(model.h, g.shape[1], garr, nparts, b))
    return list(b)


def estimate_los_points(ctl, atm, geom):
    """Estimated LOS points per ray (jur_estimate_los_points): host arithmetic, no GPU."""
    g = np.ascontiguousarray(np.asarray(geom, dtype=np.float64).T)
    z = np.ctypeslib.as_array(atm.z)[:atm.np]
    garr = (dp * 7)(*[_p(g[k]) for k in range(7)])
    out = np.zeros(g.shape[1])
    _chk(lib().jur_estimate_los_points(ctl.rayds, ctl.raydz, float(z.min()), float(z.max()), g.shape[1], garr, _p(out)))
    return out


def balance_rays(ctl, atm, geom, nparts):
    """Boundaries of nparts contiguous ray ranges with equal estimated LOS points (jur_balance_rays): no GPU."""
    g = np.ascontiguousarray(np.asarray(geom, dtype=np.float64).T)
    z = np.ctypeslib.as_array(atm.z)[:atm.np]
    garr = (dp * 7)(*[_p(g[k]) for k in range(7)])
    b = (C.c_long * (nparts + 1))()
    _chk(lib().jur_balance_rays(ctl.rayds, ctl.raydz, float(z.min()), float(z.max()), g.shape[1], garr, nparts, b))
    return list(b)


def models_set_atm(models, atm):
    _chk(lib().jur_models_set_atm(_handles(models), len(models), C.byref(atm)))


def formod_host_multi(models, geom, rad_in=None):
    """jur_formod_host_multi: the rays of one call dealt to several models (one per device).  Same result dict as
    Model.formod_host."""
    g = np.ascontiguousarray(np.asarray(geom, dtype=np.float64).T)
    nr, nd = g.shape[1], models[0].nd
    rad = np.zeros((nr, nd)) if rad_in is None else np.ascontiguousarray(rad_in, dtype=np.float64).copy()
    tau = np.zeros((nr, nd))
    tp = np.zeros((3, nr))
    npts = np.zeros(nr, dtype=np.int32)
    garr = (dp * 7)(*[_p(g[k]) for k in range(7)])
    tarr = (dp * 3)(*[_p(tp[k]) for k in range(3)])
    _chk(lib().jur_formod_host_multi(_handles(models), len(models), nr, garr, _p(rad), _p(tau), tarr,
                                     npts.ctypes.data_as(C.POINTER(C.c_int))))
    return dict(rad=rad, tau=tau, tp=np.ascontiguousarray(tp.T), np=npts)


def formod_device_multi(models, nr, d_geom, d_rad, d_tau, d_tp, d_np=0, d_status=0, stream=0, bounds=None):
    """jur_formod_device_multi: raw device addresses on models[0]'s GPU; bounds: nmodel + 1 ray indices or None."""
    b = None if bounds is None else (C.c_long * (len(models) + 1))(*bounds)
    _chk(lib().jur_formod_device_multi(_handles(models), len(models), nr, b, d_geom, d_rad, d_tau, d_tp, d_np, d_status, stream))


def formod(ctl, atm, obs):
    """Drop-in entry (reference CPUdrivers.c:179): tables from ctl.tblbase files."""
    lib().formod(C.byref(ctl), C.byref(atm), C.byref(obs))


def formod_contrib(ctl, atm, obs):
    """Drop-in formod_contrib(): obs as formod() leaves it; -> list of ng + 1 obs_t (emitters, then EXTINCT)."""
    out = (abi.obs_t * (ctl.ng + 1))()
    lib().formod_contrib(C.byref(ctl), C.byref(atm), C.byref(obs), out)
    return list(out)


def dropin_finalize():
    """Free the lanes and tables behind formod() (jur_dropin_finalize) -> number of lanes freed."""
    return lib().jur_dropin_finalize()


def track_profiles(atm):
    """jur_track_profiles: the profile table of a satellite track (IP 2; the rule in jurassic_hip.h), host only
    -> dict(first, len, block_of (nprof,), x1 (nprof, 3)); JurassicError with upstream's words for a refused track."""
    cap = atm.np // 2 + 1
    first, length, block = (np.zeros(cap, dtype=np.int32) for _ in range(3))
    x1 = np.zeros((cap, 3))
    ip_ = C.POINTER(C.c_int)
    n = _chk(lib().jur_track_profiles(C.byref(atm), first.ctypes.data_as(ip_), length.ctypes.data_as(ip_), _p(x1), block.ctypes.data_as(ip_)))
    return dict(first=first[:n], len=length[:n], block_of=block[:n], x1=x1[:n])


def cloud_points(atm):
    """jur_cloud_points: x1 = geo2cart(0, lon, lat) of every point of a cloud (IP 3; rule 3 in jurassic_hip.h), host
    only -> (np, 3)"""
    x1 = np.zeros((max(int(atm.np), 1), 3))
    n = _chk(lib().jur_cloud_points(C.byref(atm), _p(x1)))
    return x1[:n]


def cloud_lds_points():
    """jur_cloud_lds_points: the largest slice the IP 3 tracer stages in LDS"""
    return int(lib().jur_cloud_lds_points())


def intpol_atm(ctl, dest, src, device=0):
    """Regrid src onto dest's points (reference intpol_atm, jurassic.c:675): fills dest.p, t, q, k."""
    _chk(lib().jur_intpol_atm(C.byref(ctl), C.byref(dest), C.byref(src), device))


def formod_fov(ctl, obs):
    """Drop-in field-of-view convolution (reference jurassic.c:214): shape file named by ctl.fov."""
    lib().formod_fov(C.byref(ctl), C.byref(obs))


def fov_read_shape(path):
    dz, w = np.zeros(abi.NSHAPE), np.zeros(abi.NSHAPE)
    n = C.c_int(0)
    _chk(lib().jur_fov_read_shape(path.encode(), C.byref(n), _p(dz), _p(w)))
    return dz[:n.value].copy(), w[:n.value].copy()


def fov_apply(time, vpz, rad, tau, dz, w):
    """Field-of-view convolution on flat arrays, in place: rad/tau (nr, nd) C-contiguous float64."""
    time, vpz, dz, w = (np.ascontiguousarray(a, dtype=np.float64) for a in (time, vpz, dz, w))
    assert rad.flags.c_contiguous and tau.flags.c_contiguous and rad.dtype == np.float64 and rad.shape == tau.shape
    nr, nd = rad.shape
    _chk(lib().jur_fov_apply(nd, nr, _p(time), _p(vpz), _p(rad), _p(tau), nd, len(dz), _p(dz), _p(w)))


def scene_fov_live(time, rad_in):
    """The effective mask of the scene entries under a field of view (jur_scene_fov_live; host arithmetic): time (nr,),
    rad_in (nr, nd) -> live (nr, nd) bool, True where rad_in is finite in that channel on every ray of the ray's window.
    Raises JurassicError for a time stamp in two separate runs or a window of fewer than two rays."""
    time = np.ascontiguousarray(time, dtype=np.float64)
    rad = np.ascontiguousarray(rad_in, dtype=np.float64)
    if rad.ndim != 2 or rad.shape[0] != len(time) or rad.shape[1] < 1:
        raise ValueError("rad_in must be (%d, nd)" % len(time))
    live = np.zeros(rad.shape, dtype=np.uint8)
    n = _chk(lib().jur_scene_fov_live(rad.shape[1], len(time), _p(time), _p(rad), live.ctypes.data_as(C.POINTER(C.c_ubyte))))
    assert n == int(live.sum())
    return live.astype(bool)


def _pass_args(nr, time):
    if time is None:
        return None, None
    time = np.ascontiguousarray(time, dtype=np.float64)
    if time.shape != (nr,):
        raise ValueError("time must be (%d,)" % nr)
    return time, _p(time)


def scene_passes(rowptr, cap, time=None):
    """The passes of the Jacobian entries of a scene (jur_scene_passes; host arithmetic, no GPU): rowptr (nr + 1,) as
    scene_layout gives it, cap >= 1 slots per pass, time (nr,) while a field of view is set -> (pass, nmax, kmax): the
    boundaries (npass + 1,) int64, first 0 and last nr, and the slots and block columns of the largest pass."""
    rp = np.ascontiguousarray(rowptr, dtype=np.int64)
    nr = len(rp) - 1
    time, tp = _pass_args(nr, time)
    lp_ = C.POINTER(C.c_long)
    pas = np.zeros(nr + 1, dtype=np.int64)
    nmax, kmax = C.c_long(0), C.c_long(0)
    n = _chk(lib().jur_scene_passes(nr, rp.ctypes.data_as(lp_), int(cap), tp, pas.ctypes.data_as(lp_), C.byref(nmax), C.byref(kmax)))
    return pas[:n + 1].copy(), nmax.value, kmax.value


def trial_passes(nr, ntrial, cap, time=None):
    """The trial passes of a scene (jur_trial_passes; host arithmetic, no GPU): ntrial slots per ray -> (pass, nmax) as
    scene_passes."""
    time, tp = _pass_args(nr, time)
    pas = np.zeros(nr + 1, dtype=np.int64)
    nmax = C.c_long(0)
    n = _chk(lib().jur_trial_passes(nr, int(ntrial), int(cap), tp, pas.ctypes.data_as(C.POINTER(C.c_long)), C.byref(nmax)))
    return pas[:n + 1].copy(), nmax.value


def scene_pass_reserve(rowptr, cap, ntrial, time=None):
    """What Model.retrieve_scene allocates for its passes (jur_scene_pass_reserve; host arithmetic, no GPU) -> (slots,
    cols): bounds for every pass of either kind, cut anew on the rays that ended slices leave."""
    rp = np.ascontiguousarray(rowptr, dtype=np.int64)
    nr = len(rp) - 1
    time, tp = _pass_args(nr, time)
    slots, cols = C.c_long(0), C.c_long(0)
    _chk(lib().jur_scene_pass_reserve(nr, rp.ctypes.data_as(C.POINTER(C.c_long)), int(cap), int(ntrial), tp, C.byref(slots), C.byref(cols)))
    return slots.value, cols.value


def scene_recomp_offsets(rowptr, sid, then, now, nd):
    """Where a reuse iteration of Model.retrieve_scene finds the retained blocks (jur_scene_recomp_offsets; host
    arithmetic, no GPU): rowptr (nr + 1,), sid (nr,) as scene_layout and scene_slices give them, then and now (nslice,)
    the states of the slices (0: active) at the Jacobian iteration and now -> the first double of the block of every ray
    that is active now, in ray order."""
    rp = np.ascontiguousarray(rowptr, dtype=np.int64)
    nr = len(rp) - 1
    sd, th, nw = (np.ascontiguousarray(x, dtype=np.int32) for x in (sid, then, now))
    if sd.shape != (nr,) or th.shape != nw.shape:
        raise ValueError("sid must be (%d,), then and now of one shape" % nr)
    koff = np.zeros(max(nr, 1), dtype=np.int64)
    ip_, lp_ = C.POINTER(C.c_int), C.POINTER(C.c_long)
    n = _chk(lib().jur_scene_recomp_offsets(nr, rp.ctypes.data_as(lp_), sd.ctypes.data_as(ip_), th.ctypes.data_as(ip_),
                                            nw.ctypes.data_as(ip_), int(nd), koff.ctypes.data_as(lp_)))
    return koff[:n].copy()


def formod_pencil(ctl, atm, obs, ir):
    lib().formod_pencil(C.byref(ctl), C.byref(atm), C.byref(obs), ir)


def tune_trace(lanes_per_ray=0):
    """Process-wide: lanes per ray of the batched ray tracer (0: chosen per launch)."""
    lib().jur_tune_trace(lanes_per_ray)


def tune_trace_slice(mode=0):
    """Process-wide: profile slice of the batched ray tracer in LDS (0: chosen per launch, 1: never, 2: wherever it fits)."""
    lib().jur_tune_trace_slice(mode)


def tune_block_order(mode=0):
    """Process-wide: longest blocks of a sorted launch first (0: chosen per call, 1: never, 2: whenever the rays were sorted
    and the call is one trace launch)."""
    lib().jur_tune_block_order(mode)


def tune_block_order_ega(mode=-1):
    """Process-wide: the look-up kernel takes the launch's block order too (1), or runs in slot order (0, the default);
    < 0: back to JUR_BLOCK_ORDER_EGA."""
    lib().jur_tune_block_order_ega(mode)


def tune_k_elision(mode=-1):
    """Process-wide: no extinction work for an atmosphere without extinction (1, the default), or always the full work
    (0); < 0: back to JUR_K_ELISION."""
    lib().jur_tune_k_elision(mode)


ATM_CALLER, ATM_PERTURBED, ATM_DEVICE = 0, 1, 2


def atm_k_zero(k, atm_sorted=True, origin=ATM_CALLER):
    """jur_atm_k_zero: may the kernels leave the extinction values `k` (any shape, float64) out?"""
    k = np.ascontiguousarray(k, dtype=np.float64)
    return bool(lib().jur_atm_k_zero(k.ctypes.data_as(C.POINTER(C.c_double)), k.size, int(bool(atm_sorted)), int(origin)))


def tune_combine(channels_per_group=4, sync_segments=8, min_lanes=1_000_000):
    """Process-wide arrangement of the radiance-update kernel of the batched path (jur_tune_combine)."""
    lib().jur_tune_combine(channels_per_group, sync_segments, min_lanes)
