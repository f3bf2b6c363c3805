"""ctypes binding of libfakepta_amd.so (C-ABI declared in include/fakepta_amd.h).

The product path has no CPU fallback: if the library is missing this module raises at
import, and if no MI355X is visible the first compute call raises FptaError.
"""
import ctypes
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_DEFAULT_LIB = os.path.join(_HERE, "lib", "libfakepta_amd.so")
LIB_PATH = os.environ.get("FAKEPTA_AMD_LIB", _DEFAULT_LIB)

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"fakepta_amd: HIP library not found at {LIB_PATH}. Build it with "
        "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C fakepta_amd/csrc`).")

_lib = ctypes.CDLL(LIB_PATH)

_c_int = ctypes.c_int
_i32, _i64, _u64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64
_dbl = ctypes.c_double
_vp = ctypes.c_void_p
_ctx_p = ctypes.c_void_p

# (name, restype, argtypes) — mirrors include/fakepta_amd.h
_SIGS = [
    ("fpta_version", _c_int, []),
    ("fpta_create", _c_int, [_c_int, ctypes.POINTER(_ctx_p)]),
    ("fpta_destroy", _c_int, [_ctx_p]),
    ("fpta_last_error", ctypes.c_char_p, [_ctx_p]),
    ("fpta_device_count", _c_int, [ctypes.POINTER(_c_int)]),
    ("fpta_gp_accumulate", _c_int, [_ctx_p, _i64, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _dbl, _vp]),
    ("fpta_gp_accumulate_array", _c_int, [_ctx_p, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                          _dbl, _vp]),
    ("fpta_common_accumulate", _c_int, [_ctx_p, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _dbl, _dbl, _vp, _vp, _vp,
                                        _vp]),
    ("fpta_cw_accumulate", _c_int, [_ctx_p, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _dbl, _vp]),
    ("fpta_batch_cw_accumulate", _c_int, [_ctx_p, _vp, _vp, _i64, _i32, _vp, _vp, _dbl]),
    ("fpta_ephem_kepler", _c_int, [_ctx_p, _i64, _vp, _vp, _vp]),
    ("fpta_ephem_orbits", _c_int, [_ctx_p, _i64, _vp, _i32, _vp, _vp, _vp]),
    ("fpta_roemer_accumulate", _c_int, [_ctx_p, _i32, _vp, _vp, _vp, _i32, _vp, _dbl, _i32, _vp]),
    ("fpta_batch_roemer_accumulate", _c_int, [_ctx_p, _vp, _i32, _vp, _vp, _dbl]),
    ("fpta_healpix_pix2ang_ring", _c_int, [_i32, _i64, _vp, _vp, _vp]),
    ("fpta_orf_anisotropic", _c_int, [_ctx_p, _i32, _vp, _i32, _i32, _vp, _vp]),
    ("fpta_orf_plan", _c_int, [_i32, _i32, _i64, _i32, _i64, _vp]),
    ("fpta_batch_set_timing_model", _c_int, [_ctx_p, _i32, _vp, _vp, _vp, _dbl, _vp]),
    ("fpta_batch_project", _c_int, [_ctx_p]),
    ("fpta_tm_project", _c_int, [_ctx_p, _i32, _vp, _vp, _i32, _vp, _vp, _dbl, _i32, _vp, _vp]),
    ("fpta_batch_set_fit", _c_int, [_ctx_p, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _dbl, _vp, _vp]),
    ("fpta_batch_fit_info", _c_int, [_ctx_p, _vp]),
    ("fpta_batch_fit", _c_int, [_ctx_p, _vp]),
    ("fpta_batch_fit_cross", _c_int, [_ctx_p, _vp]),
    ("fpta_fit_coefficients", _c_int, [_ctx_p, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp,
                                       _vp, _dbl, _i32, _vp, _vp, _vp, _vp]),
    ("fpta_batch_set_os", _c_int, [_ctx_p, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp,
                                   _dbl, _i32, _vp, _vp, _vp]),
    ("fpta_batch_os_info", _c_int, [_ctx_p, _vp]),
    ("fpta_batch_os", _c_int, [_ctx_p, _vp, _vp, _vp]),
    ("fpta_os_statistic", _c_int, [_ctx_p, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp,
                                   _i32, _vp, _vp, _vp, _dbl, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("fpta_batch_set_os_scrambles", _c_int, [_ctx_p, _i32, _vp, _vp, _vp, _vp]),
    ("fpta_batch_os_scrambles_info", _c_int, [_ctx_p, _vp]),
    ("fpta_batch_os_scrambles", _c_int, [_ctx_p, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("fpta_os_scrambles", _c_int, [_ctx_p, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp,
                                    _i32, _vp, _vp, _vp, _dbl, _i32, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp,
                                    _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("fpta_os_scramble_match", _c_int, [_ctx_p, _i32, _i32, _vp, _i32, _vp, _vp, _vp]),
    ("fpta_batch_set_os_spectra", _c_int, [_ctx_p, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp, _vp,
                                           _i32, _vp, _vp, _vp, _dbl, _i32, _vp, _i32, _vp]),
    ("fpta_batch_os_spectra", _c_int, [_ctx_p, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("fpta_batch_set_lnl", _c_int, [_ctx_p, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _dbl,
                                    _i32, _vp, _vp, _vp]),
    ("fpta_batch_lnl_info", _c_int, [_ctx_p, _vp]),
    ("fpta_batch_lnl", _c_int, [_ctx_p, _vp, _vp, _vp]),
    ("fpta_lnl_grid", _c_int, [_ctx_p, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _vp,
                               _vp, _vp, _dbl, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("fpta_batch_set_fe", _c_int, [_ctx_p, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _dbl, _i32,
                                   _vp, _i32, _vp, _vp, _dbl, _vp, _vp, _vp, _vp, _vp]),
    ("fpta_batch_fe_info", _c_int, [_ctx_p, _vp]),
    ("fpta_batch_fe", _c_int, [_ctx_p, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("fpta_fe_statistic", _c_int, [_ctx_p, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp,
                                   _vp, _vp, _dbl, _i32, _vp, _i32, _vp, _vp, _dbl, _i32, _vp, _vp, _vp, _vp, _vp, _vp,
                                   _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("fpta_batch_set_clnl", _c_int, [_ctx_p, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _dbl,
                                     _i32, _vp, _i32, _vp, _vp, _vp]),
    ("fpta_batch_clnl_info", _c_int, [_ctx_p, _vp]),
    ("fpta_batch_clnl", _c_int, [_ctx_p, _vp, _vp, _vp, _vp]),
    ("fpta_clnl_grid", _c_int, [_ctx_p, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _vp,
                                _vp, _vp, _dbl, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("fpta_white_accumulate", _c_int, [_ctx_p, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    ("fpta_gp_covariance", _c_int, [_ctx_p, _i64, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("fpta_noise_wiener", _c_int, [_ctx_p, _i64, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("fpta_noise_draw", _c_int, [_ctx_p, _i64, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _i64, _i32,
                                 _vp]),
    ("fpta_batch_set_toas", _c_int, [_ctx_p, _i32, _vp, _vp, _vp]),
    ("fpta_batch_add_signal", _c_int, [_ctx_p, _i32, _i32, _vp, _vp, _dbl, _dbl, _vp, _vp]),
    ("fpta_batch_set_white", _c_int, [_ctx_p, _vp, _i64, _vp, _vp, _vp]),
    ("fpta_batch_clear_signals", _c_int, [_ctx_p]),
    ("fpta_batch_synth", _c_int, [_ctx_p, _u64, _i64, _i32, _vp, _vp]),
    ("fpta_batch_synth_spectra", _c_int, [_ctx_p, _u64, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("fpta_batch_synth_from_z", _c_int, [_ctx_p, _i32, _i32, _vp, _vp]),
    ("fpta_batch_download", _c_int, [_ctx_p, _i32, _i32, _vp]),
    ("fpta_batch_device_out", _c_int, [_ctx_p, ctypes.POINTER(_vp), ctypes.POINTER(_i64), ctypes.POINTER(_i32)]),
    ("fpta_batch_checksums", _c_int, [_ctx_p, _vp]),
    ("fpta_batch_synth_checksums", _c_int, [_ctx_p, _u64, _i64, _i64, _i32, _vp]),
    ("fpta_batch_correlations", _c_int, [_ctx_p, _i32, _vp]),
    ("fpta_batch_info", _c_int, [_ctx_p, _vp]),
    ("fpta_batch_grid_info", _c_int, [_ctx_p, _vp]),
    ("fpta_batch_grid_info_n", _c_int, [_ctx_p, _vp, _i32]),
    ("fpta_set_option", _c_int, [_ctx_p, _i32, _i64]),
    ("fpta_kernel_stats", _c_int, [_ctx_p, _i32, ctypes.POINTER(_i64), ctypes.POINTER(_dbl)]),
    ("fpta_reset_stats", _c_int, [_ctx_p]),
    ("fpta_synchronize", _c_int, [_ctx_p]),
    ("fpta_debug_philox", _c_int, [_ctx_p, _i64, _vp, _vp, _vp]),
    ("fpta_debug_normals", _c_int, [_ctx_p, _i64, _vp, _vp]),
    ("fpta_debug_fill_out", _c_int, [_ctx_p, _dbl]),
    ("fpta_debug_fused_shape", _c_int, [_ctx_p, _vp]),
    ("fpta_debug_dense", _c_int, [_ctx_p, _i32, _i64, _i64, _vp]),
    ("fpta_get_option", _c_int, [_ctx_p, _i32, ctypes.POINTER(_i64)]),
    ("fpta_build_flags", _c_int, []),
    ("fpta_batch_path_reason", ctypes.c_char_p, [_ctx_p]),
    ("fpta_multi_create", _c_int, [_i32, _vp, ctypes.POINTER(_vp)]),
    ("fpta_multi_destroy", _c_int, [_vp]),
    ("fpta_multi_last_error", ctypes.c_char_p, [_vp]),
    ("fpta_multi_size", _c_int, [_vp]),
    ("fpta_multi_context", _ctx_p, [_vp, _i32]),
    ("fpta_multi_set_toas", _c_int, [_vp, _i32, _vp, _vp, _vp]),
    ("fpta_multi_add_signal", _c_int, [_vp, _i32, _i32, _vp, _vp, _dbl, _dbl, _vp, _vp]),
    ("fpta_multi_set_white", _c_int, [_vp, _vp, _i64, _vp, _vp, _vp]),
    ("fpta_multi_set_option", _c_int, [_vp, _i32, _i64]),
    ("fpta_multi_synth", _c_int, [_vp, _u64, _i64, _i64, _i32, _vp]),
    ("fpta_multi_set_gather", _c_int, [_vp, _i32]),
    ("fpta_multi_last_gather", _c_int, [_vp]),
    ("fpta_comm_unique_id", _c_int, [_vp]),
    ("fpta_comm_init_rank", _c_int, [_ctx_p, _i32, _i32, _vp, ctypes.POINTER(_vp)]),
    ("fpta_comm_destroy", _c_int, [_vp]),
    ("fpta_comm_last_error", ctypes.c_char_p, [_vp]),
    ("fpta_comm_size", _c_int, [_vp, ctypes.POINTER(_i32), ctypes.POINTER(_i32)]),
    ("fpta_comm_max", _c_int, [_vp, ctypes.POINTER(_dbl)]),
    ("fpta_comm_gather", _c_int, [_vp, _vp, _i64, _vp]),
]
# entry points newer than an older library a same-box A/B may load through FAKEPTA_AMD_LIB (tools/gpu_ab_cfg.sh LIB=):
# bound when present (the product library exports every one: tests/test_capi_symbols.py)
_OPTIONAL = {"fpta_debug_normals", "fpta_debug_fused_shape", "fpta_debug_dense"}
for _name, _res, _args in _SIGS:
    try:
        _fn = getattr(_lib, _name)
    except AttributeError:
        if _name in _OPTIONAL and LIB_PATH != _DEFAULT_LIB:
            continue
        raise
    _fn.restype = _res
    _fn.argtypes = _args

EXPORTED = [s[0] for s in _SIGS]

OPT_SYNTH_PATH, OPT_MFMA_MIN_REAL, OPT_PROFILE, OPT_ANCHOR, OPT_VALU_VARIANT, OPT_FUSE_WHITE = 1, 2, 3, 4, 5, 6
OPT_GRID_WIDTH, OPT_GRID_SIGMA, OPT_GRID_MFMA, OPT_FUSE_CHECKSUMS = 7, 8, 9, 10
OPT_MIX_MFMA, OPT_OVERLAP, OPT_INTERP_LDS, OPT_GRID_COALESCE, OPT_INTERP_WS, OPT_SIDE_SPLIT = 11, 12, 13, 14, 15, 16
OPT_DFT_GEN, OPT_GEN_MIX, OPT_ASYNC_SUMS, OPT_PART_GROUP, OPT_INTERP_PSR, OPT_INTERP_WR = 17, 18, 19, 20, 21, 22
OPT_INTERP_FUSED, OPT_FUSED_NEXT_MIX, OPT_CW_SPLIT, OPT_ORF_SPLIT = 23, 25, 26, 27  # key 24 is retired
OPT_ROEMER_CHUNK = 28
OPTIONS = (OPT_SYNTH_PATH, OPT_MFMA_MIN_REAL, OPT_PROFILE, OPT_ANCHOR, OPT_VALU_VARIANT, OPT_FUSE_WHITE,
           OPT_GRID_WIDTH, OPT_GRID_SIGMA, OPT_GRID_MFMA, OPT_FUSE_CHECKSUMS, OPT_MIX_MFMA, OPT_OVERLAP,
           OPT_INTERP_LDS, OPT_GRID_COALESCE, OPT_INTERP_WS, OPT_SIDE_SPLIT, OPT_DFT_GEN, OPT_GEN_MIX,
           OPT_ASYNC_SUMS, OPT_PART_GROUP, OPT_INTERP_PSR, OPT_INTERP_WR, OPT_INTERP_FUSED, OPT_FUSED_NEXT_MIX,
           OPT_CW_SPLIT, OPT_ORF_SPLIT, OPT_ROEMER_CHUNK)
K_GEN, K_MIX, K_SYNTH, K_WHITE, K_DENSE, K_GRID, K_CW, K_EPHEM = 0, 1, 2, 3, 4, 5, 6, 7
CW_NPAR = 9  # FPTA_CW_NPAR: cos_gwtheta, gwphi, cos_inc, log10_mc, log10_fgw, log10_h, phase0, psi, psrterm
EPHEM_NBODY = 14  # FPTA_EPHEM_NBODY: mass, T, then (value, rate per century) of inc, Om, omega, a, e, l0
ROEMER_NPAR = 22  # FPTA_ROEMER_NPAR: a body, d_mass, d_Om, d_omega, d_inc, d_a, d_e, d_l0, 1 / mass_ss
EPHEM_E_MAX = 0.95  # FPTA_EPHEM_E_MAX
EPHEM_MSUN = 1.327124400e20 / 6.6743e-11  # FPTA_EPHEM_MSUN
TM_MAX_COL = 16  # columns of one pulsar's design matrix (fpta_tm_project, fpta_batch_set_timing_model)
FIT_MAX_COMP, FIT_MAX_COEF = 4, 512  # components and Fourier columns of one fit (fpta_batch_set_fit)
OS_MAX_COMP, OS_MAX_COL, OS_MAX_COEF = 8, 1024, 512  # components, all Fourier columns, the target's (fpta_batch_set_os)
SCR_MAX, SCR_MAX_BYTES, SCR_PAIR_PAD = 65536, 8 << 30, 16  # scrambles, bytes of their pair rows (fpta_batch_set_os_scrambles)
OSS_MAX_VARY, OSS_MAX_COL = 4, 128  # varied components and their Fourier columns (fpta_batch_set_os_spectra)
LNL_MAX_COEF, LNL_MAX_GRID = 256, 4096  # the target's Fourier columns and the grid points (fpta_batch_set_lnl)
CLNL_MAX_ORF, CLNL_MAX_N, CLNL_BUDGET = 8, 16384, 32 << 30  # ORFs, n = P K and cached bytes (fpta_batch_set_clnl)
FE_MAX_COMP, FE_MAX_FREQ, FE_MAX_SKY, FE_MAX_PSR = 7, 256, 12288, 256  # fpta_batch_set_fe's limits
ORF_PLAN_LEN = 10  # FPTA_ORF_PLAN_LEN
ORF_PLAN_KEYS = ("tile", "chunk", "map_group", "n_tiles", "n_chunks", "n_split", "chunks_per_split", "n_groups",
                 "groups_per_launch", "workspace_bytes")


def interp_kernel_name(code):
    """The gridded interpolation kernel of the last block (fpta_batch_grid_info_n slot 15: 1 + 4 kind + 2 white +
    partial checksums), as rocprofv3 names it; None before any gridded block."""
    if code <= 0:
        return None
    kind, white, part = (code - 1) >> 2, "true" if (code - 1) & 2 else "false", "true" if (code - 1) & 1 else "false"
    if kind >= INTERP_KIND_FUSED0:  # launch_grid_fused's instance table
        i = kind - INTERP_KIND_FUSED0
        return FUSED_KERNELS[i] if i < len(FUSED_KERNELS) else None
    return {0: f"k_grid_interp_mfma<{white}, {part}, 8>", 1: f"k_grid_interp_ws<{part}>",
            2: f"k_grid_interp_ws2<{part}>", 3: f"k_grid_interp_lds<{white}, {part}>",
            4: f"k_grid_interp_st<{white}, {part}>", 5: f"k_grid_interp_u<{part}>",
            6: f"k_grid_interp_psr<{part}, 4>", 7: f"k_grid_interp_psr<{part}, 8>",
            10: "k_grid_interp_wr"}.get(kind)


# k_grid_fused<NQ, ODD, GEN, HALF> instances in launch_grid_fused's order (capi_host.h kInterpKindFused0 + index)
INTERP_KIND_FUSED0 = 11
FUSED_KERNELS = tuple(f"k_grid_fused<{nq}, {odd}, {gen}, {half}>" for nq, half in ((8, "false"), (12, "false"), (8, "true"))
                      for odd, gen in (("false", "false"), ("false", "true"), ("true", "true")))
BUILD_DEBUG, BUILD_DIAG = 1, 2
GATHER_AUTO, GATHER_RCCL, GATHER_HOST = 0, 1, 2
COMM_ID_BYTES = 128


def build_flags():
    """FPTA_BUILD_DEBUG (1) when the loaded library is the debug build (make debug), FPTA_BUILD_DIAG (2) when it
    holds the diagnostic kernels (make variant DEFS=-DFPTA_DIAG_KERNELS)."""
    return int(_lib.fpta_build_flags())


class FptaError(RuntimeError):
    pass


def pix2ang_ring(nside, ipix=None):
    """(theta, phi) of the HEALPix RING pixels ipix (default: all 12 nside^2) (fpta_healpix_pix2ang_ring). Host only:
    needs no context and no GPU."""
    nside = int(nside)
    if ipix is None:
        if not 1 <= nside <= 1024:  # the library's own range, checked before the pixel list is sized by it
            raise FptaError(f"fpta_healpix_pix2ang_ring failed (-22): nside {nside} outside [1, 1024]")
        ipix = np.arange(12 * nside * nside, dtype=np.int64)
    ipix = np.ascontiguousarray(ipix, dtype=np.int64)
    theta, phi = np.empty(ipix.shape), np.empty(ipix.shape)
    rc = _lib.fpta_healpix_pix2ang_ring(nside, ipix.size, _ptr(ipix), _ptr(theta), _ptr(phi))
    if rc < 0:
        raise FptaError(f"fpta_healpix_pix2ang_ring failed ({rc}): {_lib.fpta_last_error(None).decode()}")
    return theta, phi


def orf_plan(n_psr, nside, n_map=1, split=0, npix=None):
    """The launch plan of fpta_orf_anisotropic for a shape (fpta_orf_plan), as a dict of ORF_PLAN_KEYS. Host only. It
    also checks the shape: FptaError for a bad nside or npix != 12 nside^2."""
    info = np.zeros(ORF_PLAN_LEN, dtype=np.int64)
    npix = 12 * int(nside) * int(nside) if npix is None else int(npix)
    rc = _lib.fpta_orf_plan(int(n_psr), int(nside), npix, int(n_map), int(split), _ptr(info))
    if rc < 0:
        raise FptaError(f"fpta_orf_plan failed ({rc}): {_lib.fpta_last_error(None).decode()}")
    return dict(zip(ORF_PLAN_KEYS, (int(v) for v in info)))


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_vp)


class Context:
    """One device context (one GPU, one HIP stream). Not thread-safe: one per thread/process."""

    def __init__(self, device=0):
        h = _ctx_p()
        rc = _lib.fpta_create(int(device), ctypes.byref(h))
        if rc != 0:
            raise FptaError(f"fpta_create(device={device}) failed ({rc}): "
                            f"{_lib.fpta_last_error(None).decode()}")
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            _lib.fpta_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc < 0:
            raise FptaError(f"{what} failed ({rc}): {_lib.fpta_last_error(self._h).decode()}")
        return rc

    # --------------------------------------------------------------- drop-in
    def gp_accumulate(self, toas, nu, segments, residuals, sign=1.0, masks=None):
        """segments: list of (f, ccos, csin, idx, freqf). residuals: float64 array updated in place."""
        toas, nu = _f64(toas), _f64(nu)
        n = len(toas)
        assert residuals.dtype == np.float64 and residuals.flags.c_contiguous and len(residuals) == n
        nm = np.array([len(s[0]) for s in segments], dtype=np.int32)
        f = _f64(np.concatenate([np.asarray(s[0], float) for s in segments]))
        cc = _f64(np.concatenate([np.asarray(s[1], float) for s in segments]))
        cs = _f64(np.concatenate([np.asarray(s[2], float) for s in segments]))
        idx = _f64([s[3] for s in segments])
        ff = _f64([s[4] for s in segments])
        m = None
        if masks is not None and any(x is not None for x in masks):
            m = np.ones((len(segments), n), dtype=np.uint8)
            for i, x in enumerate(masks):
                if x is not None:
                    m[i] = np.asarray(x, dtype=bool)
        self._check(_lib.fpta_gp_accumulate(self._h, n, _ptr(toas), _ptr(nu), len(segments), _ptr(nm), _ptr(f),
                                            _ptr(cc), _ptr(cs), _ptr(idx), _ptr(ff), _ptr(m), float(sign),
                                            _ptr(residuals)), "fpta_gp_accumulate")

    # ------------------------------------------------------------------ dense covariance
    @staticmethod
    def _dense_args(toas, nu, segments, white_var):
        """segments: list of (f [N], w = psd * df [N], idx, freqf)."""
        toas, nu = _f64(toas), _f64(nu)
        n = len(toas)
        assert len(nu) == n and len(segments) > 0
        nm = np.array([len(s[0]) for s in segments], dtype=np.int32)
        for s in segments:
            assert len(s[1]) == len(s[0])
        f = _f64(np.concatenate([np.asarray(s[0], float) for s in segments]))
        w = _f64(np.concatenate([np.asarray(s[1], float) for s in segments]))
        idx = _f64([s[2] for s in segments])
        ff = _f64([s[3] for s in segments])
        wv = None if white_var is None else _f64(white_var)
        if wv is not None:
            assert len(wv) == n
        keep = (toas, nu, nm, f, w, idx, ff, wv)
        args = (n, _ptr(toas), _ptr(nu), len(segments), _ptr(nm), _ptr(f), _ptr(w), _ptr(idx), _ptr(ff), _ptr(wv))
        return n, keep, args

    def gp_covariance(self, toas, nu, segments, white_var=None):
        """sum_s B_s diag(psd df) B_s^T (+ diag(white_var)) as a [n, n] float64 array."""
        n, keep, args = self._dense_args(toas, nu, segments, white_var)
        cov = np.empty((n, n), dtype=np.float64)
        self._check(_lib.fpta_gp_covariance(self._h, *args, _ptr(cov)), "fpta_gp_covariance")
        self._dense_shape = (n, 0)
        del keep
        return cov

    def noise_wiener(self, toas, nu, segments, white_var, residuals):
        """red_cov C^-1 residuals with C = red_cov + diag(white_var) (device Cholesky)."""
        n, keep, args = self._dense_args(toas, nu, segments, white_var)
        r = _f64(residuals)
        assert len(r) == n
        out = np.empty(n, dtype=np.float64)
        self._check(_lib.fpta_noise_wiener(self._h, *args, _ptr(r), _ptr(out)), "fpta_noise_wiener")
        self._dense_shape = (n, 0)
        del keep
        return out

    def noise_draw(self, toas, nu, segments, white_var, seed, real0, n_real):
        """[n_real, n] draws of N(0, red_cov + diag(white_var)) (Philox stream, device Cholesky)."""
        n, keep, args = self._dense_args(toas, nu, segments, white_var)
        out = np.empty((n_real, n), dtype=np.float64)
        self._check(_lib.fpta_noise_draw(self._h, *args, int(seed) & 0xFFFFFFFFFFFFFFFF, int(real0), int(n_real),
                                         _ptr(out)), "fpta_noise_draw")
        self._dense_shape = (n, int(n_real))
        del keep
        return out

    def debug_dense(self, what):
        """What the last dense call of this context left on the device (fpta_debug_dense): what = 0 the matrix [n, n]
        (after noise_wiener / noise_draw the Cholesky factor in its lower triangle), 1 the solve's y [n] (after
        noise_wiener), 2 the normals [n, n_real] of the last noise_draw. FptaError when that call left no such item."""
        n, n_real = getattr(self, "_dense_shape", (0, 0))
        rows, cols = n, {0: n, 1: 1, 2: n_real}.get(int(what), 0)
        out = np.empty((rows, cols) if rows * cols else (1, 1), dtype=np.float64)  # empty: the library refuses
        self._check(_lib.fpta_debug_dense(self._h, int(what), rows, cols, _ptr(out)), "fpta_debug_dense")
        return out[:, 0].copy() if what == 1 else out

    def gp_accumulate_array(self, offs, toas, nu, segments, residuals, sign=1.0, masks=None):
        """Array form: segments = list of (f [P, N], ccos [P, N], csin [P, N], idx, freqf);
        masks: None or list (per segment) of None / bool [n_toa_total]. residuals updated in place."""
        offs = np.ascontiguousarray(offs, dtype=np.int64)
        toas, nu = _f64(toas), _f64(nu)
        P, n = len(offs) - 1, int(offs[-1])
        assert residuals.dtype == np.float64 and residuals.flags.c_contiguous and len(residuals) == n
        for s in segments:
            assert np.shape(s[0]) == np.shape(s[1]) == np.shape(s[2]) and np.shape(s[0])[0] == P
        nm = np.array([np.shape(s[0])[1] for s in segments], dtype=np.int32)
        f = _f64(np.concatenate([np.asarray(s[0], float).ravel() for s in segments]))
        cc = _f64(np.concatenate([np.asarray(s[1], float).ravel() for s in segments]))
        cs = _f64(np.concatenate([np.asarray(s[2], float).ravel() for s in segments]))
        idx = _f64([s[3] for s in segments])
        ff = _f64([s[4] for s in segments])
        m = None
        if masks is not None and any(x is not None for x in masks):
            m = np.ones((len(segments), n), dtype=np.uint8)
            for i, x in enumerate(masks):
                if x is not None:
                    m[i] = np.asarray(x, dtype=bool)
        self._check(_lib.fpta_gp_accumulate_array(self._h, P, _ptr(offs), _ptr(toas), _ptr(nu), len(segments),
                                                  _ptr(nm), _ptr(f), _ptr(cc), _ptr(cs), _ptr(idx), _ptr(ff), _ptr(m),
                                                  float(sign), _ptr(residuals)), "fpta_gp_accumulate_array")

    def common_accumulate(self, offs, toas, nu, f, amp, idx, freqf, L, z, residuals, want_x=True):
        offs = np.ascontiguousarray(offs, dtype=np.int64)
        toas, nu, f, amp, L, z = map(_f64, (toas, nu, f, amp, L, z))
        P = len(offs) - 1
        N = len(f)
        assert z.shape == (N, 2, P) and L.shape == (P, P) and len(residuals) == offs[-1]
        x = np.empty((N, 2, P)) if want_x else None
        self._check(_lib.fpta_common_accumulate(self._h, P, _ptr(offs), _ptr(toas), _ptr(nu), N, _ptr(f), _ptr(amp),
                                                float(idx), float(freqf), _ptr(L), _ptr(z), _ptr(residuals),
                                                _ptr(x)), "fpta_common_accumulate")
        return x

    def cw_accumulate(self, offs, toas, pos, pdist_s, sources, residuals, sign=1.0):
        """Continuous waves of circular binaries summed into every pulsar (fpta_cw_accumulate). pos [P, 3] unit
        vectors, pdist_s [P] pulsar distances in light-seconds, sources [S, CW_NPAR]; residuals updated in place."""
        offs = np.ascontiguousarray(offs, dtype=np.int64)
        toas, pos, pdist_s = _f64(toas), _f64(pos), _f64(pdist_s)
        sources = _f64(sources).reshape(-1, CW_NPAR)
        P, n = len(offs) - 1, int(offs[-1])
        if not (isinstance(residuals, np.ndarray) and residuals.dtype == np.float64 and residuals.flags.c_contiguous
                and residuals.flags.writeable and residuals.shape == (n,)):
            raise ValueError(f"cw_accumulate: residuals must be a writable contiguous float64 array of {n} values")
        if len(toas) != n or pos.shape != (P, 3) or pdist_s.shape != (P,):
            raise ValueError(f"cw_accumulate: expected {n} toas, pos [{P}, 3] and pdist_s [{P}]")
        self._check(_lib.fpta_cw_accumulate(self._h, P, _ptr(offs), _ptr(toas), _ptr(pos), _ptr(pdist_s),
                                            len(sources), _ptr(sources), float(sign), _ptr(residuals)),
                    "fpta_cw_accumulate")

    def batch_cw_accumulate(self, pos, pdist_s, n_tab, src_offs, sources, sign=1.0):
        """Continuous waves added to every realization of the last batch block, in place on the device
        (fpta_batch_cw_accumulate). pos [P, 3] and pdist_s [P] or [R, P] (light-seconds) for the batch layout's
        pulsars; n_tab 1 (one table for all) or R tables in CSR form: table r is sources[src_offs[r]:src_offs[r + 1]],
        rows of CW_NPAR values (fakepta_amd.cw.population_tables makes the three)."""
        P = self.batch_info()["n_psr"]
        if P == 0:  # no layout to check the shapes against: the library's own state error
            raise FptaError("fpta_batch_cw_accumulate failed (-77): batch_cw_accumulate: set_toas first")
        pos, pdist_s = _f64(pos), _f64(pdist_s)
        src_offs = np.ascontiguousarray(src_offs, dtype=np.int64)
        sources = _f64(sources).reshape(-1, CW_NPAR)
        n_tab = int(n_tab)
        if pos.shape != (P, 3) or pdist_s.ndim not in (1, 2) or pdist_s.shape[-1] != P:
            raise ValueError(f"batch_cw_accumulate: expected pos [{P}, 3] and pdist_s [{P}] or [n_real, {P}], got "
                             f"{pos.shape} and {pdist_s.shape}")
        if pdist_s.ndim == 2:
            try:
                _, _, R = self.batch_device_out()
            except FptaError:
                R = pdist_s.shape[0]  # no block: the library's state error follows
            if pdist_s.shape[0] != R:
                raise ValueError(f"batch_cw_accumulate: pdist_s for {pdist_s.shape[0]} realizations, the block has {R}")
        if n_tab < 0 or src_offs.shape != (n_tab + 1,) or (len(src_offs) and src_offs[-1] != len(sources)):
            raise ValueError(f"batch_cw_accumulate: src_offs must hold {n_tab + 1} offsets ending at the "
                             f"{len(sources)} source rows")
        self._check(_lib.fpta_batch_cw_accumulate(self._h, _ptr(pos), _ptr(pdist_s), P if pdist_s.ndim == 2 else 0,
                                                  n_tab, _ptr(src_offs), _ptr(sources), float(sign)),
                    "fpta_batch_cw_accumulate")

    def ephem_kepler(self, M, e):
        """E with E - e sin E = M, elementwise (fpta_ephem_kepler); M and e broadcast against each other."""
        M, e = np.broadcast_arrays(np.asarray(M, dtype=np.float64), np.asarray(e, dtype=np.float64))
        shape = M.shape
        M, e = _f64(M).ravel(), _f64(e).ravel()
        out = np.empty(M.size)
        self._check(_lib.fpta_ephem_kepler(self._h, M.size, _ptr(M), _ptr(e), _ptr(out)), "fpta_ephem_kepler")
        return out.reshape(shape)

    def ephem_orbits(self, toas, bodies, planets=True, sun=False):
        """(planetssb [n, B, 6] or None, sunssb [n, 3] or None) of the body table [B, EPHEM_NBODY] at the TOAs
        (fpta_ephem_orbits)."""
        toas = _f64(toas).ravel()
        bodies = _f64(bodies).reshape(-1, EPHEM_NBODY)
        if not (planets or sun):
            raise ValueError("ephem_orbits: ask for planets, sun or both")
        # zero-filled: with no TOAs or no bodies the call writes nothing
        pssb = np.zeros((len(toas), len(bodies), 6)) if planets else None
        sssb = np.zeros((len(toas), 3)) if sun else None
        self._check(_lib.fpta_ephem_orbits(self._h, len(toas), _ptr(toas), len(bodies), _ptr(bodies), _ptr(pssb),
                                           _ptr(sssb)), "fpta_ephem_orbits")
        return pssb, sssb

    def roemer_accumulate(self, offs, toas, pos, rows, out, sign=1.0, separate=False):
        """Roemer delays of the rows [R, ROEMER_NPAR] for every pulsar (fpta_roemer_accumulate). pos [P, 3]; out
        [n] updated in place (out += sign * sum of the rows' delays), or with separate [R, n] written."""
        offs = np.ascontiguousarray(offs, dtype=np.int64)
        toas, pos = _f64(toas), _f64(pos)
        rows = _f64(rows).reshape(-1, ROEMER_NPAR)
        P, n = len(offs) - 1, int(offs[-1])
        shape = (len(rows), n) if separate else (n,)
        if not (isinstance(out, np.ndarray) and out.dtype == np.float64 and out.flags.c_contiguous
                and out.flags.writeable and out.shape == shape):
            raise ValueError(f"roemer_accumulate: out must be a writable contiguous float64 array of shape {shape}")
        if len(toas) != n or pos.shape != (P, 3):
            raise ValueError(f"roemer_accumulate: expected {n} toas and pos [{P}, 3]")
        self._check(_lib.fpta_roemer_accumulate(self._h, P, _ptr(offs), _ptr(toas), _ptr(pos), len(rows), _ptr(rows),
                                                float(sign), int(bool(separate)), _ptr(out)),
                    "fpta_roemer_accumulate")

    def batch_roemer_accumulate(self, pos, n_tab, row_offs, rows, sign=1.0):
        """Roemer delays of ephemeris errors added to every realization of the last batch block, in place on the
        device (fpta_batch_roemer_accumulate). pos [P, 3] for the batch layout's pulsars; n_tab 1 (one table for all)
        or R tables in CSR form: table r is rows[row_offs[r]:row_offs[r + 1]], rows of ROEMER_NPAR values
        (fakepta_amd.ephem.perturbation_tables makes the three)."""
        P = self.batch_info()["n_psr"]
        if P == 0:  # no layout to check the shapes against: the library's own state error
            raise FptaError("fpta_batch_roemer_accumulate failed (-77): batch_roemer_accumulate: set_toas first")
        pos = _f64(pos)
        row_offs = np.ascontiguousarray(row_offs, dtype=np.int64)
        rows = _f64(rows).reshape(-1, ROEMER_NPAR)
        n_tab = int(n_tab)
        if pos.shape != (P, 3):
            raise ValueError(f"batch_roemer_accumulate: expected pos [{P}, 3], got {pos.shape}")
        if n_tab < 0 or row_offs.shape != (n_tab + 1,) or (len(row_offs) and row_offs[-1] != len(rows)):
            raise ValueError(f"batch_roemer_accumulate: row_offs must hold {n_tab + 1} offsets ending at the "
                             f"{len(rows)} rows")
        self._check(_lib.fpta_batch_roemer_accumulate(self._h, _ptr(pos), n_tab, _ptr(row_offs), _ptr(rows),
                                                      float(sign)), "fpta_batch_roemer_accumulate")

    def orf_anisotropic(self, pos, nside, h_maps, out=None):
        """ORFs [M, P, P] of the maps h_maps [M, 12 nside^2] (HEALPix RING) for pulsars at the unit vectors pos [P, 3]
        (fpta_orf_anisotropic). out: a contiguous float64 [M, P, P] to write into (left untouched by a refused call)."""
        pos, h_maps = _f64(pos), _f64(h_maps)
        if pos.ndim != 2 or pos.shape[1] != 3 or h_maps.ndim != 2:
            raise ValueError("orf_anisotropic: expected pos [P, 3] and h_maps [M, npix]")
        P, (M, npix) = len(pos), h_maps.shape
        orf_plan(P, nside, M, self.get_option(OPT_ORF_SPLIT), npix=npix)  # the shape: nside, the map length
        if out is None:
            out = np.empty((M, P, P))
        elif not (isinstance(out, np.ndarray) and out.dtype == np.float64 and out.flags.c_contiguous
                  and out.flags.writeable and out.shape == (M, P, P)):
            raise ValueError(f"orf_anisotropic: out must be a writable contiguous float64 array of shape {(M, P, P)}")
        self._check(_lib.fpta_orf_anisotropic(self._h, P, _ptr(pos), int(nside), M, _ptr(h_maps), _ptr(out)),
                    "fpta_orf_anisotropic")
        return out

    @staticmethod
    def _tm_args(what, P, n, M, ncol_psr, weights, rcond=None):
        """The design matrix [n, n_col] (None: no column), column counts [P] or None, weights [n] or None and rcond
        (None: the library's default, 0) of a call that fits a design out, as contiguous arrays of the C types and a
        float."""
        M = np.zeros((n, 0)) if M is None else _f64(M)
        if M.ndim != 2 or M.shape[0] != n or M.shape[1] > TM_MAX_COL:
            raise ValueError(f"{what}: M must be [{n}, n_col <= {TM_MAX_COL}], got {M.shape}")
        if ncol_psr is not None:
            ncol_psr = np.ascontiguousarray(ncol_psr, dtype=np.int32)
            if ncol_psr.shape != (P,):
                raise ValueError(f"{what}: ncol_psr must hold {P} column counts")
        if weights is not None:
            weights = _f64(weights)
            if weights.shape != (n,):
                raise ValueError(f"{what}: weights must hold {n} values")
        return M, ncol_psr, weights, 0.0 if rcond is None else float(rcond)

    @staticmethod
    def _offs_args(what, offs):
        """The CSR offsets [P + 1] of a one-shot call as int64, with P and n_toa."""
        offs = np.ascontiguousarray(offs, dtype=np.int64)
        if offs.ndim != 1 or len(offs) < 1:
            raise ValueError(f"{what}: offs must be [P + 1]")
        return offs, len(offs) - 1, int(offs[-1])

    @classmethod
    def _oneshot_args(cls, what, offs, toas, nu, res):
        """The array and the vectors of a one-shot call that reads res [n_vec, n_toa] or [n_toa]: offs, toas, nu and res
        as contiguous arrays of the C types, with P, n_toa and n_vec."""
        offs, P, n = cls._offs_args(what, offs)
        toas, nu, res = _f64(toas), _f64(nu), _f64(res)
        if toas.shape != (n,) or nu.shape != (n,):
            raise ValueError(f"{what}: toas and nu must hold {n} values")
        if res.ndim not in (1, 2) or res.shape[-1] != n:
            raise ValueError(f"{what}: res must be [n_vec, {n}] or [{n}], got {res.shape}")
        return offs, toas, nu, res, P, n, 1 if res.ndim == 1 else res.shape[0]

    def _info4(self, fn, what):
        """The four integers of a fpta_batch_*_info call."""
        info = np.zeros(4, dtype=np.int64)
        self._check(fn(self._h, _ptr(info)), what)
        return [int(v) for v in info]

    def _block_real(self):
        """R of the resident block, or 0 without one (the library's state error follows from the call itself)."""
        try:
            return self.batch_device_out()[2]
        except FptaError:
            return 0

    def tm_project(self, offs, M, res, ncol_psr=None, weights=None, rcond=None):
        """The weighted least-squares fit of the design matrices M [n_toa, n_col] (pulsar p: rows offs[p] ..
        offs[p + 1], its leading ncol_psr[p] columns) removed from every row of res [n_vec, n_toa] or [n_toa], in place
        (fpta_tm_project). Returns the ranks [P]."""
        offs, P, n = self._offs_args("tm_project", offs)
        M, ncol_psr, weights, rcond = self._tm_args("tm_project", P, n, _f64(M), ncol_psr, weights, rcond)
        if not (isinstance(res, np.ndarray) and res.dtype == np.float64 and res.flags.c_contiguous
                and res.flags.writeable and res.ndim in (1, 2) and res.shape[-1] == n):
            raise ValueError(f"tm_project: res must be a writable contiguous float64 array [n_vec, {n}] or [{n}]")
        n_vec = 1 if res.ndim == 1 else res.shape[0]
        rank = np.zeros(P, dtype=np.int32)
        self._check(_lib.fpta_tm_project(self._h, P, _ptr(offs), _ptr(M), M.shape[1], _ptr(ncol_psr), _ptr(weights),
                                         rcond, n_vec, _ptr(res), _ptr(rank)), "fpta_tm_project")
        return rank

    def white_accumulate(self, sigma, z, residuals, blocks=None, ecorr_sigma=None, zb=None):
        sigma, z = _f64(sigma), _f64(z)
        n = len(sigma)
        nb = 0
        bo = bi = es = zbb = None
        if blocks:
            nb = len(blocks)
            bo = np.concatenate([[0], np.cumsum([len(b) for b in blocks])]).astype(np.int64)
            bi = np.concatenate([np.asarray(b, dtype=np.int64) for b in blocks]).astype(np.int64)
            es, zbb = _f64(ecorr_sigma), _f64(zb)
        self._check(_lib.fpta_white_accumulate(self._h, n, _ptr(sigma), _ptr(z), nb, _ptr(bo), _ptr(bi), _ptr(es),
                                               _ptr(zbb), _ptr(residuals)), "fpta_white_accumulate")

    # --------------------------------------------------------------- batch
    def batch_set_toas(self, offs, toas, nu):
        offs = np.ascontiguousarray(offs, dtype=np.int64)
        toas, nu = _f64(toas), _f64(nu)
        self._check(_lib.fpta_batch_set_toas(self._h, len(offs) - 1, _ptr(offs), _ptr(toas), _ptr(nu)),
                    "fpta_batch_set_toas")

    def batch_add_signal(self, kind, f, amp, idx=0.0, freqf=1400.0, L=None, mask=None):
        f, amp = _f64(f), _f64(amp)
        nm = f.shape[-1]
        L = None if L is None else _f64(L)
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        return self._check(_lib.fpta_batch_add_signal(self._h, int(kind), nm, _ptr(f), _ptr(amp), float(idx),
                                                      float(freqf), _ptr(L), _ptr(m)), "fpta_batch_add_signal")

    def batch_set_white(self, sigma=None, blocks=None, ecorr_sigma=None):
        s = None if sigma is None else _f64(sigma)
        nb = 0
        bo = bi = es = None
        if blocks:
            nb = len(blocks)
            bo = np.concatenate([[0], np.cumsum([len(b) for b in blocks])]).astype(np.int64)
            bi = np.concatenate([np.asarray(b, dtype=np.int64) for b in blocks]).astype(np.int64)
            es = _f64(ecorr_sigma)
        self._check(_lib.fpta_batch_set_white(self._h, _ptr(s), nb, _ptr(bo), _ptr(bi), _ptr(es)),
                    "fpta_batch_set_white")

    def batch_set_timing_model(self, M, ncol_psr=None, weights=None, rcond=None):
        """The timing model of the batch layout: M [n_toa, n_col] in the layout's TOA order, None or zero columns to
        clear it (fpta_batch_set_timing_model). Returns the ranks [P]."""
        info = self.batch_info()
        P, n = info["n_psr"], info["n_toa"]
        rank = np.zeros(P, dtype=np.int32)
        if P == 0:  # no layout to check M against: the library's own state error
            raise FptaError("fpta_batch_set_timing_model failed (-77): set_timing_model: set_toas first")
        M, ncol_psr, weights, rcond = self._tm_args("batch_set_timing_model", P, n, M, ncol_psr, weights, rcond)
        self._check(_lib.fpta_batch_set_timing_model(self._h, M.shape[1], _ptr(M), _ptr(ncol_psr), _ptr(weights),
                                                     rcond, _ptr(rank)), "fpta_batch_set_timing_model")
        return rank

    def batch_project(self):
        """Remove the timing-model fit from the last block, in place on the device (fpta_batch_project)."""
        self._check(_lib.fpta_batch_project(self._h), "fpta_batch_project")

    @staticmethod
    def _fit_args(what, P, n_modes, f, idx, freqf, max_comp=FIT_MAX_COMP, max_col=FIT_MAX_COEF):
        """The component tables of a Fourier-fit call as contiguous arrays of the C types: n_modes [n_comp] int32 (up
        to max_comp components and max_col columns), f [sum N_c] (common) or [P, sum N_c], idx and freqf [n_comp].
        Returns them and whether f is common."""
        n_modes = np.ascontiguousarray(n_modes, dtype=np.int32)
        if n_modes.ndim != 1 or not 1 <= len(n_modes) <= max_comp or np.any(n_modes < 1):
            raise ValueError(f"{what}: n_modes must hold 1 .. {max_comp} positive mode counts, got {n_modes}")
        n_f = int(n_modes.sum())
        if 2 * n_f > max_col:
            raise ValueError(f"{what}: {2 * n_f} Fourier columns, more than {max_col}")
        f = _f64(f)
        if f.shape not in ((n_f,), (P, n_f)):
            raise ValueError(f"{what}: f must be [{n_f}] or [{P}, {n_f}], got {f.shape}")
        idx, freqf = _f64(idx), _f64(freqf)
        if idx.shape != n_modes.shape or freqf.shape != n_modes.shape:
            raise ValueError(f"{what}: idx and freqf must hold one value per component")
        return n_modes, f, idx, freqf, f.ndim == 1

    def batch_set_fit(self, n_modes, f, idx, freqf, M=None, ncol_psr=None, weights=None, rcond=None):
        """The Fourier fit of the batch layout (fpta_batch_set_fit): components of n_modes[c] frequencies (f: one grid
        [sum N_c] for the array or [P, sum N_c]) with chromatic index idx[c] at freqf[c]; M [n_toa, n_col] the
        nuisance design that is marginalised (None: nothing). n_modes None or empty clears the fit. Returns
        (kept Fourier columns [P], kept mask [P, K] bool)."""
        info = self.batch_info()
        P, n = info["n_psr"], info["n_toa"]
        rank = np.zeros(P, dtype=np.int32)
        if P == 0 or n_modes is None or len(n_modes) == 0:  # without a layout: the library's own state error
            self._check(_lib.fpta_batch_set_fit(self._h, 0, None, None, 1, None, None, 0, None, None, None, 0.0,
                                                _ptr(rank), None), "fpta_batch_set_fit")
            return rank, np.zeros((P, 0), dtype=bool)
        n_modes, f, idx, freqf, common = self._fit_args("batch_set_fit", P, n_modes, f, idx, freqf)
        M, ncol_psr, weights, rcond = self._tm_args("batch_set_fit", P, n, M, ncol_psr, weights, rcond)
        kept = np.zeros((P, 2 * int(n_modes.sum())), dtype=np.uint8)
        self._check(_lib.fpta_batch_set_fit(self._h, len(n_modes), _ptr(n_modes), _ptr(f), int(common), _ptr(idx),
                                            _ptr(freqf), M.shape[1], _ptr(M), _ptr(ncol_psr), _ptr(weights), rcond,
                                            _ptr(rank), _ptr(kept)), "fpta_batch_set_fit")
        return rank, kept.astype(bool)

    def batch_fit_info(self):
        """K and mode count of the fit that is set (0: none), whether its grid is common, and the realizations of the
        last fit result (fpta_batch_fit_info)."""
        K, n_mode, common, n_real = self._info4(_lib.fpta_batch_fit_info, "fpta_batch_fit_info")
        return dict(K=K, n_mode=n_mode, common=bool(common), n_real=n_real)

    def batch_fit(self, K=None, to_host=True):
        """Fit the last block (fpta_batch_fit): [P, K, R] on the host, or None with the result left on the device.
        The buffer is sized from the library's own K; a K given here is only checked against it."""
        have = self.batch_fit_info()["K"]
        if K is not None and have and int(K) != have:
            raise ValueError(f"batch_fit: the fit that is set has {have} Fourier columns, not {K}")
        if not to_host:
            self._check(_lib.fpta_batch_fit(self._h, None), "fpta_batch_fit")
            return None
        out = np.empty((self.batch_info()["n_psr"], have, self._block_real()))
        self._check(_lib.fpta_batch_fit(self._h, _ptr(out)), "fpta_batch_fit")
        return out

    def batch_fit_cross(self, n_mode=None):
        """[n_mode, P, P]: per mode the sum over the last fit's realizations of cos_a cos_b + sin_a sin_b
        (fpta_batch_fit_cross; a common grid only). The buffer is sized from the library's own mode count; an n_mode
        given here is only checked against it."""
        have = self.batch_fit_info()["n_mode"]
        if n_mode is not None and have and int(n_mode) != have:
            raise ValueError(f"batch_fit_cross: the fit that is set has {have} modes, not {n_mode}")
        P = self.batch_info()["n_psr"]
        out = np.empty((have, P, P))
        self._check(_lib.fpta_batch_fit_cross(self._h, _ptr(out)), "fpta_batch_fit_cross")
        return out

    def fit_coefficients(self, offs, toas, nu, n_modes, f, idx, freqf, res, M=None, ncol_psr=None, weights=None,
                         rcond=None):
        """The Fourier coefficients of every row of res [n_vec, n_toa] or [n_toa] for any array
        (fpta_fit_coefficients). Returns (coef [P, K, n_vec], kept Fourier columns [P], kept mask [P, K] bool)."""
        offs, toas, nu, res, P, n, n_vec = self._oneshot_args("fit_coefficients", offs, toas, nu, res)
        n_modes, f, idx, freqf, common = self._fit_args("fit_coefficients", P, n_modes, f, idx, freqf)
        M, ncol_psr, weights, rcond = self._tm_args("fit_coefficients", P, n, M, ncol_psr, weights, rcond)
        K = 2 * int(n_modes.sum())
        coef = np.zeros((P, K, n_vec))
        rank, kept = np.zeros(P, dtype=np.int32), np.zeros((P, K), dtype=np.uint8)
        self._check(_lib.fpta_fit_coefficients(self._h, P, _ptr(offs), _ptr(toas), _ptr(nu), len(n_modes),
                                               _ptr(n_modes), _ptr(f), int(common), _ptr(idx), _ptr(freqf),
                                               M.shape[1], _ptr(M), _ptr(ncol_psr), _ptr(weights), rcond, n_vec,
                                               _ptr(res), _ptr(coef), _ptr(rank), _ptr(kept)), "fpta_fit_coefficients")
        return coef, rank, kept.astype(bool)

    @staticmethod
    def _phi_mask_args(what, P, n, n_modes, phi, masks):
        """phi [P, sum N_c] (a row [sum N_c] is repeated) and masks None or uint8 [C, n] (an entry None: the component
        acts everywhere) of a noise model whose component tables _fit_args has made."""
        n_f = int(n_modes.sum())
        phi = _f64(phi)
        if phi.shape == (n_f,):
            phi = np.ascontiguousarray(np.tile(phi, (P, 1)))
        if phi.shape != (P, n_f):
            raise ValueError(f"{what}: phi must be [{n_f}] or [{P}, {n_f}], got {phi.shape}")
        mask = None
        if masks is not None and any(m is not None for m in masks):
            if len(masks) != len(n_modes):
                raise ValueError(f"{what}: {len(masks)} masks for {len(n_modes)} components")
            mask = np.ones((len(n_modes), n), dtype=np.uint8)
            for c, m in enumerate(masks):
                if m is not None:
                    m = np.asarray(m)
                    if m.shape != (n,):
                        raise ValueError(f"{what}: the mask of component {c} must hold {n} flags, got {m.shape}")
                    mask[c] = m != 0
        return phi, mask

    @classmethod
    def _noise_args(cls, what, P, n, n_modes, f, idx, freqf, phi, masks):
        """A noise model without a target as contiguous arrays of the C types: the component tables as _fit_args makes
        them (up to OS_MAX_COMP components, OS_MAX_COL columns), then _phi_mask_args. Returns (n_modes, f, idx, freqf,
        common, phi, mask)."""
        n_modes, f, idx, freqf, common = cls._fit_args(what, P, n_modes, f, idx, freqf, OS_MAX_COMP, OS_MAX_COL)
        phi, mask = cls._phi_mask_args(what, P, n, n_modes, phi, masks)
        return n_modes, f, idx, freqf, common, phi, mask

    @classmethod
    def _os_args(cls, what, P, n, n_modes, f, idx, freqf, phi, masks, target, phi_hat, G):
        """The tables of an optimal-statistic call as contiguous arrays of the C types: the component tables as
        _fit_args makes them (up to OS_MAX_COMP components, OS_MAX_COL columns), phi and masks as _phi_mask_args makes
        them, phi_hat [N_target], G [J, P, P]."""
        n_modes, f, idx, freqf, common = cls._fit_args(what, P, n_modes, f, idx, freqf, OS_MAX_COMP, OS_MAX_COL)
        target = int(target)
        if not 0 <= target < len(n_modes):
            raise ValueError(f"{what}: target component {target} outside [0, {len(n_modes)})")
        if 2 * int(n_modes[target]) > OS_MAX_COEF:
            raise ValueError(f"{what}: the target has {2 * int(n_modes[target])} Fourier columns, more than "
                             f"{OS_MAX_COEF}")
        phi, mask = cls._phi_mask_args(what, P, n, n_modes, phi, masks)
        phi_hat = _f64(phi_hat)
        if phi_hat.shape != (int(n_modes[target]),):
            raise ValueError(f"{what}: the template must hold {int(n_modes[target])} values, got {phi_hat.shape}")
        G = np.zeros((0, P, P)) if G is None else _f64(G)
        if G.ndim == 2:
            G = G[None]
        if G.ndim != 3 or G.shape[1:] != (P, P):
            raise ValueError(f"{what}: G must be [J, {P}, {P}], got {G.shape}")
        return n_modes, f, idx, freqf, common, phi, mask, target, phi_hat, np.ascontiguousarray(G)

    def batch_set_os(self, n_modes, f, idx, freqf, phi, target, phi_hat, G, masks=None, M=None, ncol_psr=None,
                     weights=None, rcond=None):
        """The optimal statistic of the batch layout (fpta_batch_set_os): the noise model's components (n_modes, f, idx,
        freqf as batch_set_fit; phi [P, sum N_c] or [sum N_c] prior variances; masks None or one entry per component),
        the target component and its template phi_hat [N], the pair-weight matrices G [J, P, P], the marginalised
        design M and the weights. n_modes None or empty clears it. Returns (kept columns of M [P], N_ab [P, P])."""
        info = self.batch_info()
        P, n = info["n_psr"], info["n_toa"]
        rank = np.zeros(P, dtype=np.int32)
        if P == 0 or n_modes is None or len(n_modes) == 0:  # without a layout: the library's own state error
            self._check(_lib.fpta_batch_set_os(self._h, 0, None, None, 1, None, None, None, None, 0, None, 0, None,
                                               None, None, 0.0, 0, None, _ptr(rank), None), "fpta_batch_set_os")
            return rank, np.zeros((P, P))
        n_modes, f, idx, freqf, common, phi, mask, target, phi_hat, G = self._os_args(
            "batch_set_os", P, n, n_modes, f, idx, freqf, phi, masks, target, phi_hat, G)
        M, ncol_psr, weights, rcond = self._tm_args("batch_set_os", P, n, M, ncol_psr, weights, rcond)
        nab = np.zeros((P, P))
        self._check(_lib.fpta_batch_set_os(self._h, len(n_modes), _ptr(n_modes), _ptr(f), int(common), _ptr(idx),
                                           _ptr(freqf), _ptr(phi), _ptr(mask), target, _ptr(phi_hat), M.shape[1],
                                           _ptr(M), _ptr(ncol_psr), _ptr(weights), rcond, len(G), _ptr(G), _ptr(rank),
                                           _ptr(nab)), "fpta_batch_set_os")
        return rank, nab

    def batch_os_info(self):
        """K, N and J of the optimal statistic that is set (0: none) and the realizations of the last result
        (fpta_batch_os_info)."""
        return dict(zip(("K", "N", "J", "n_real"), self._info4(_lib.fpta_batch_os_info, "fpta_batch_os_info")))

    def batch_os(self, per_mode=False, coefficients=False):
        """The optimal statistic of the last block (fpta_batch_os): (Q [J, R], Q_mode [J, N, R] or None, X [P, K, R] or
        None). The buffers are sized from the library's own K, N and J."""
        have, R = self.batch_os_info(), self._block_real()
        Q = np.empty((have["J"], R))
        Qm = np.empty((have["J"], have["N"], R)) if per_mode else None
        X = np.empty((self.batch_info()["n_psr"], have["K"], R)) if coefficients else None
        self._check(_lib.fpta_batch_os(self._h, _ptr(Q), _ptr(Qm), _ptr(X)), "fpta_batch_os")
        return Q, Qm, X

    @staticmethod
    def _scramble_args(what, P, pos, G):
        """The scrambles of a call as contiguous float64: positions [J, P, 3] or matrices [J, P, P], exactly one of
        them. Returns (J, pos or None, G or None)."""
        if (pos is None) == (G is None):
            raise ValueError(f"{what}: exactly one of positions and matrices must be given")
        if pos is not None:
            pos = _f64(pos)
            if pos.ndim != 3 or pos.shape[1:] != (P, 3):
                raise ValueError(f"{what}: positions must be [J, {P}, 3], got {pos.shape}")
            return len(pos), pos, None
        G = _f64(G)
        if G.ndim == 2:
            G = np.ascontiguousarray(G[None])
        if G.ndim != 3 or G.shape[1:] != (P, P):
            raise ValueError(f"{what}: matrices must be [J, {P}, {P}], got {G.shape}")
        return len(G), None, G

    def batch_set_os_scrambles(self, pos=None, G=None):
        """The sky scrambles of the batch layout's optimal statistic (fpta_batch_set_os_scrambles): fictitious
        positions pos [J, P, 3] (unit vectors; their Hellings-Downs matrices are made on the device) or explicit
        symmetric matrices G [J, P, P]. Neither, or an empty one, clears them. Returns (norm [J], match [J, n_g])
        against the n_g matrices of the statistic that is set."""
        have = self.batch_os_info()
        n_g = have["J"]
        if have["K"] == 0:  # no statistic: the library's own state error
            self._check(_lib.fpta_batch_set_os_scrambles(self._h, 1, None, None, None, None),
                        "fpta_batch_set_os_scrambles")
        if (pos is None and G is None) or len(pos if pos is not None else G) == 0:
            self._check(_lib.fpta_batch_set_os_scrambles(self._h, 0, None, None, None, None),
                        "fpta_batch_set_os_scrambles")
            return np.zeros(0), np.zeros((0, n_g))
        J, pos, G = self._scramble_args("batch_set_os_scrambles", self.batch_info()["n_psr"], pos, G)
        norm, match = np.zeros(J), np.zeros((J, n_g))
        self._check(_lib.fpta_batch_set_os_scrambles(self._h, J, _ptr(pos), _ptr(G), _ptr(norm), _ptr(match)),
                    "fpta_batch_set_os_scrambles")
        return norm, match

    def batch_os_scrambles_info(self):
        """The scrambles that are set (0: none), the matrices of their statistic, the pairs of a row and the
        realizations of the last result (fpta_batch_os_scrambles_info)."""
        return dict(zip(("n_scr", "n_g", "n_pair", "n_real"),
                        self._info4(_lib.fpta_batch_os_scrambles_info, "fpta_batch_os_scrambles_info")))

    def batch_os_scrambles(self, full=False):
        """The scrambled statistic of the last block (fpta_batch_os_scrambles): a dict of snr_obs [n_g, R], count_ge
        [n_g, R] int64, mean, std and max [R] of the null and, with full=True, snr_null [J, R]. The buffers are sized
        from the library's own counts."""
        have, R = self.batch_os_scrambles_info(), self._block_real()
        out = dict(snr_obs=np.zeros((have["n_g"], R)), count_ge=np.zeros((have["n_g"], R), dtype=np.int64),
                   mean=np.zeros(R), std=np.zeros(R), max=np.zeros(R),
                   snr_null=np.zeros((have["n_scr"], R)) if full else None)
        self._check(_lib.fpta_batch_os_scrambles(self._h, _ptr(out["snr_obs"]), _ptr(out["count_ge"]),
                                                 _ptr(out["mean"]), _ptr(out["std"]), _ptr(out["max"]),
                                                 _ptr(out["snr_null"])), "fpta_batch_os_scrambles")
        return out

    def os_scrambles(self, offs, toas, nu, n_modes, f, idx, freqf, phi, target, phi_hat, G, res, pos=None,
                     matrices=None, masks=None, M=None, ncol_psr=None, weights=None, rcond=None, full=False):
        """The scrambled optimal statistic of every row of res [n_vec, n_toa] or [n_toa] for any array
        (fpta_os_scrambles): os_statistic's arguments and the scrambles as batch_set_os_scrambles takes them. A dict:
        batch_os_scrambles' entries (with full=True also Qs [J, n_vec], the numerators of snr_null), Q [n_g, n_vec],
        X [P, K, n_vec], norm [J], match [J, n_g] and N_ab [P, P]."""
        offs, toas, nu, res, P, n, n_vec = self._oneshot_args("os_scrambles", offs, toas, nu, res)
        n_modes, f, idx, freqf, common, phi, mask, target, phi_hat, G = self._os_args(
            "os_scrambles", P, n, n_modes, f, idx, freqf, phi, masks, target, phi_hat, G)
        M, ncol_psr, weights, rcond = self._tm_args("os_scrambles", P, n, M, ncol_psr, weights, rcond)
        J, pos, matrices = self._scramble_args("os_scrambles", P, pos, matrices)
        N, n_g = int(n_modes[target]), len(G)
        out = dict(snr_obs=np.zeros((n_g, n_vec)), count_ge=np.zeros((n_g, n_vec), dtype=np.int64),
                   mean=np.zeros(n_vec), std=np.zeros(n_vec), max=np.zeros(n_vec),
                   snr_null=np.zeros((J, n_vec)) if full else None, Qs=np.zeros((J, n_vec)) if full else None,
                   Q=np.zeros((n_g, n_vec)),
                   X=np.zeros((P, 2 * N, n_vec)), norm=np.zeros(J), match=np.zeros((J, n_g)), N_ab=np.zeros((P, P)))
        self._check(_lib.fpta_os_scrambles(
            self._h, P, _ptr(offs), _ptr(toas), _ptr(nu), len(n_modes), _ptr(n_modes), _ptr(f), int(common), _ptr(idx),
            _ptr(freqf), _ptr(phi), _ptr(mask), target, _ptr(phi_hat), M.shape[1], _ptr(M), _ptr(ncol_psr),
            _ptr(weights), rcond, n_g, _ptr(G), J, _ptr(pos), _ptr(matrices), n_vec, _ptr(res), _ptr(out["Q"]),
            _ptr(out["X"]), _ptr(out["norm"]), _ptr(out["match"]), _ptr(out["snr_obs"]), _ptr(out["count_ge"]),
            _ptr(out["mean"]), _ptr(out["std"]), _ptr(out["max"]), _ptr(out["snr_null"]), _ptr(out["Qs"]),
            _ptr(out["N_ab"])),
            "fpta_os_scrambles")
        return out

    def os_scramble_match(self, pos, ref, rows=False):
        """match [J, n_ref] of the Hellings-Downs matrices of the positions pos [J, P, 3] against the reference
        matrices ref [n_ref, P, P] or [P, P] (fpta_os_scramble_match): sum G_ref G / sqrt(sum G_ref^2 sum G^2) over
        the pairs. rows=True: (match, the device's pair rows [J, P (P - 1) / 2] in np.tril_indices(P, -1) order)."""
        ref = _f64(ref)
        if ref.ndim == 2:
            ref = np.ascontiguousarray(ref[None])
        if ref.ndim != 3 or ref.shape[1] != ref.shape[2]:
            raise ValueError(f"os_scramble_match: the reference must be [n_ref, P, P], got {ref.shape}")
        J, pos, _ = self._scramble_args("os_scramble_match", ref.shape[1], pos, None)
        P = ref.shape[1]
        match = np.zeros((J, len(ref)))
        out = np.zeros((J, P * (P - 1) // 2)) if rows else None
        self._check(_lib.fpta_os_scramble_match(self._h, P, J, _ptr(pos), len(ref), _ptr(ref), _ptr(match), _ptr(out)),
                    "fpta_os_scramble_match")
        return (match, out) if rows else match

    def batch_set_os_spectra(self, n_modes, f, idx, freqf, phi, target, phi_hat, vary, vary_seg, G, n_orf, masks=None,
                             M=None, ncol_psr=None, weights=None, rcond=None):
        """The optimal statistic under a spectrum per realization of the batch layout (fpta_batch_set_os_spectra): the
        noise model, target, template, design and weights as batch_set_os takes them; vary the component indices of
        the varied set (the target last) and vary_seg the layout signal of each; the first n_orf of G [J, P, P] get a
        joint normal matrix. n_modes None or empty clears it. Returns the kept columns of M [P]."""
        info = self.batch_info()
        P, n = info["n_psr"], info["n_toa"]
        rank = np.zeros(P, dtype=np.int32)
        if P == 0 or n_modes is None or len(n_modes) == 0:  # without a layout: the library's own state error
            self._check(_lib.fpta_batch_set_os_spectra(self._h, 0, None, None, 1, None, None, None, None, 0, None, 0,
                                                       None, None, 0, None, None, None, 0.0, 0, None, 0, _ptr(rank)),
                        "fpta_batch_set_os_spectra")
            return rank
        n_modes, f, idx, freqf, common, phi, mask, target, phi_hat, G = self._os_args(
            "batch_set_os_spectra", P, n, n_modes, f, idx, freqf, phi, masks, target, phi_hat, G)
        M, ncol_psr, weights, rcond = self._tm_args("batch_set_os_spectra", P, n, M, ncol_psr, weights, rcond)
        vary = np.ascontiguousarray(vary, dtype=np.int32).reshape(-1)
        vary_seg = np.ascontiguousarray(vary_seg, dtype=np.int32).reshape(-1)
        if len(vary) != len(vary_seg):
            raise ValueError("batch_set_os_spectra: vary and vary_seg must have one entry per varied component")
        q = 2 * int(sum(int(n_modes[v]) for v in vary if 0 <= v < len(n_modes)))
        if q > OSS_MAX_COL:
            raise ValueError(f"batch_set_os_spectra: the varied set has {q} Fourier columns, more than {OSS_MAX_COL}")
        self._check(_lib.fpta_batch_set_os_spectra(
            self._h, len(n_modes), _ptr(n_modes), _ptr(f), int(common), _ptr(idx), _ptr(freqf), _ptr(phi), _ptr(mask),
            target, _ptr(phi_hat), len(vary), _ptr(vary), _ptr(vary_seg), M.shape[1], _ptr(M), _ptr(ncol_psr),
            _ptr(weights), rcond, len(G), _ptr(G), int(n_orf), _ptr(rank)), "fpta_batch_set_os_spectra")
        return rank

    def batch_os_spectra(self, seg, form, per_pulsar, tables, K, J, n_orf, per_mode=False, coefficients=False,
                         pair_norms=False, zp=False):
        """The statistic of the last block under the tables of batch_synth_spectra's form (fpta_batch_os_spectra): a dict
        of Q [J, R], norm [J, R], joint [n_orf, n_orf, R] and, on request, Q_mode [J, N, R], X [P, K, R], N_ab [R, P, P]
        (the entries a >= b) and Zp [R, P, K, K]. K, J and n_orf are those of the statistic that is set."""
        R, P, N = self._block_real(), self.batch_info()["n_psr"], K // 2
        tables = [_f64(t) for t in tables]
        n = len(tables)
        if not (len(seg) == len(form) == len(per_pulsar) == n):
            raise ValueError("batch_os_spectra: seg, form, per_pulsar and tables must have one entry per table")
        seg, form, per = (np.ascontiguousarray(v, dtype=np.int32).reshape(n) for v in (seg, form, per_pulsar))
        rows = np.array([t.shape[0] if t.ndim else 0 for t in tables], dtype=np.int32)
        ptrs = (_vp * max(n, 1))(*[t.ctypes.data for t in tables])
        out = dict(Q=np.zeros((J, R)), norm=np.zeros((J, R)), joint=np.zeros((n_orf, n_orf, R)),
                   Q_mode=np.zeros((J, N, R)) if per_mode else None, X=np.zeros((P, K, R)) if coefficients else None,
                   N_ab=np.zeros((R, P, P)) if pair_norms else None, Zp=np.zeros((R, P, K, K)) if zp else None)
        self._check(_lib.fpta_batch_os_spectra(self._h, n, _ptr(seg), _ptr(form), _ptr(per), _ptr(rows),
                                               ctypes.cast(ptrs, _vp), _ptr(out["Q"]), _ptr(out["Q_mode"]),
                                               _ptr(out["X"]), _ptr(out["norm"]), _ptr(out["joint"]),
                                               _ptr(out["N_ab"]), _ptr(out["Zp"])), "fpta_batch_os_spectra")
        return out

    def os_statistic(self, offs, toas, nu, n_modes, f, idx, freqf, phi, target, phi_hat, G, res, masks=None, M=None,
                     ncol_psr=None, weights=None, rcond=None):
        """The optimal statistic of every row of res [n_vec, n_toa] or [n_toa] for any array (fpta_os_statistic).
        Returns (Q [J, n_vec], Q_mode [J, N, n_vec], X [P, K, n_vec], kept columns of M [P], N_ab [P, P])."""
        offs, toas, nu, res, P, n, n_vec = self._oneshot_args("os_statistic", offs, toas, nu, res)
        n_modes, f, idx, freqf, common, phi, mask, target, phi_hat, G = self._os_args(
            "os_statistic", P, n, n_modes, f, idx, freqf, phi, masks, target, phi_hat, G)
        M, ncol_psr, weights, rcond = self._tm_args("os_statistic", P, n, M, ncol_psr, weights, rcond)
        N = int(n_modes[target])
        Q, Qm, X = np.zeros((len(G), n_vec)), np.zeros((len(G), N, n_vec)), np.zeros((P, 2 * N, n_vec))
        rank, nab = np.zeros(P, dtype=np.int32), np.zeros((P, P))
        self._check(_lib.fpta_os_statistic(self._h, P, _ptr(offs), _ptr(toas), _ptr(nu), len(n_modes), _ptr(n_modes),
                                           _ptr(f), int(common), _ptr(idx), _ptr(freqf), _ptr(phi), _ptr(mask), target,
                                           _ptr(phi_hat), M.shape[1], _ptr(M), _ptr(ncol_psr), _ptr(weights), rcond,
                                           len(G), _ptr(G), n_vec, _ptr(res), _ptr(Q), _ptr(Qm), _ptr(X), _ptr(rank),
                                           _ptr(nab)), "fpta_os_statistic")
        return Q, Qm, X, rank, nab

    @classmethod
    def _lnl_args(cls, what, P, n, n_modes, f, idx, freqf, phi, masks, target, phi_grid):
        """The tables of a likelihood-grid call: _os_args' (without a template and pair weights) and phi_grid [G, N]
        (a row [N] is one grid point) within the library's limits."""
        n_modes = np.ascontiguousarray(n_modes, dtype=np.int32)
        t = int(target)
        N = int(n_modes[t]) if n_modes.ndim == 1 and 0 <= t < len(n_modes) else 1
        n_modes, f, idx, freqf, common, phi, mask, target, _, _ = cls._os_args(
            what, P, n, n_modes, f, idx, freqf, phi, masks, target, np.ones(N), None)
        if 2 * N > LNL_MAX_COEF:
            raise ValueError(f"{what}: the target has {2 * N} Fourier columns, more than {LNL_MAX_COEF}")
        phi_grid = _f64(phi_grid)
        if phi_grid.ndim == 1:
            phi_grid = phi_grid[None]
        if phi_grid.ndim != 2 or phi_grid.shape[1] != N:
            raise ValueError(f"{what}: the grid must be [G, {N}], got {phi_grid.shape}")
        if not 1 <= len(phi_grid) <= LNL_MAX_GRID:
            raise ValueError(f"{what}: {len(phi_grid)} grid points outside [1, {LNL_MAX_GRID}]")
        return n_modes, f, idx, freqf, common, phi, mask, target, np.ascontiguousarray(phi_grid)

    def batch_set_lnl(self, n_modes, f, idx, freqf, phi, target, phi_grid, masks=None, M=None, ncol_psr=None,
                      weights=None, rcond=None):
        """The likelihood grid of the batch layout (fpta_batch_set_lnl): the noise model as batch_set_os takes it, the
        target component (its own phi is not part of the base model) and phi_grid [G, N], the target's prior variance
        per grid point and mode. n_modes None or empty clears it. Returns (kept columns of M [P], ld [P, G])."""
        info = self.batch_info()
        P, n = info["n_psr"], info["n_toa"]
        rank = np.zeros(P, dtype=np.int32)
        if P == 0 or n_modes is None or len(n_modes) == 0:  # without a layout: the library's own state error
            self._check(_lib.fpta_batch_set_lnl(self._h, 0, None, None, 1, None, None, None, None, 0, 0, None, None,
                                                None, 0.0, 0, None, _ptr(rank), None), "fpta_batch_set_lnl")
            return rank, np.zeros((P, 0))
        n_modes, f, idx, freqf, common, phi, mask, target, phi_grid = self._lnl_args(
            "batch_set_lnl", P, n, n_modes, f, idx, freqf, phi, masks, target, phi_grid)
        M, ncol_psr, weights, rcond = self._tm_args("batch_set_lnl", P, n, M, ncol_psr, weights, rcond)
        ld = np.zeros((P, len(phi_grid)))
        self._check(_lib.fpta_batch_set_lnl(self._h, len(n_modes), _ptr(n_modes), _ptr(f), int(common), _ptr(idx),
                                            _ptr(freqf), _ptr(phi), _ptr(mask), target, M.shape[1], _ptr(M),
                                            _ptr(ncol_psr), _ptr(weights), rcond, len(phi_grid), _ptr(phi_grid),
                                            _ptr(rank), _ptr(ld)), "fpta_batch_set_lnl")
        return rank, ld

    def batch_lnl_info(self):
        """K, N and G of the likelihood grid that is set (0: none) and the realizations of the last result
        (fpta_batch_lnl_info)."""
        return dict(zip(("K", "N", "G", "n_real"), self._info4(_lib.fpta_batch_lnl_info, "fpta_batch_lnl_info")))

    def batch_lnl(self, per_pulsar=False, coefficients=False):
        """The likelihood grid of the last block (fpta_batch_lnl): (dlnL [G, R], q_psr [P, G, R] or None, X [P, K, R] or
        None). The buffers are sized from the library's own K and G."""
        have, R = self.batch_lnl_info(), self._block_real()
        P = self.batch_info()["n_psr"]
        d = np.empty((have["G"], R))
        q = np.empty((P, have["G"], R)) if per_pulsar else None
        X = np.empty((P, have["K"], R)) if coefficients else None
        self._check(_lib.fpta_batch_lnl(self._h, _ptr(d), _ptr(q), _ptr(X)), "fpta_batch_lnl")
        return d, q, X

    def lnl_grid(self, offs, toas, nu, n_modes, f, idx, freqf, phi, target, phi_grid, res, masks=None, M=None,
                 ncol_psr=None, weights=None, rcond=None, factors=False):
        """The likelihood grid of every row of res [n_vec, n_toa] or [n_toa] for any array (fpta_lnl_grid). Returns
        (dlnL [G, n_vec], q_psr [P, G, n_vec], X [P, K, n_vec], kept columns of M [P], ld [P, G], U [P, G, K, K] (the
        plan's fp64 factors) or None)."""
        offs, toas, nu, res, P, n, n_vec = self._oneshot_args("lnl_grid", offs, toas, nu, res)
        n_modes, f, idx, freqf, common, phi, mask, target, phi_grid = self._lnl_args(
            "lnl_grid", P, n, n_modes, f, idx, freqf, phi, masks, target, phi_grid)
        M, ncol_psr, weights, rcond = self._tm_args("lnl_grid", P, n, M, ncol_psr, weights, rcond)
        K, G = 2 * int(n_modes[target]), len(phi_grid)
        d, q, X = np.zeros((G, n_vec)), np.zeros((P, G, n_vec)), np.zeros((P, K, n_vec))
        rank, ld = np.zeros(P, dtype=np.int32), np.zeros((P, G))
        U = np.zeros((P, G, K, K)) if factors else None
        self._check(_lib.fpta_lnl_grid(self._h, P, _ptr(offs), _ptr(toas), _ptr(nu), len(n_modes), _ptr(n_modes),
                                       _ptr(f), int(common), _ptr(idx), _ptr(freqf), _ptr(phi), _ptr(mask), target,
                                       M.shape[1], _ptr(M), _ptr(ncol_psr), _ptr(weights), rcond, G, _ptr(phi_grid),
                                       n_vec, _ptr(res), _ptr(d), _ptr(q), _ptr(X), _ptr(rank), _ptr(ld), _ptr(U)),
                    "fpta_lnl_grid")
        return d, q, X, rank, ld, U

    @classmethod
    def _clnl_args(cls, what, P, n, n_modes, f, idx, freqf, phi, masks, target, phi_grid, A):
        """The tables of a correlated-likelihood call: _lnl_args' and the ORF factors A [n_orf, P, P] (one [P, P] is
        one ORF) within the library's limits."""
        out = cls._lnl_args(what, P, n, n_modes, f, idx, freqf, phi, masks, target, phi_grid)
        A = _f64(A)
        if A.ndim == 2:
            A = A[None]
        if A.ndim != 3 or A.shape[1:] != (P, P):
            raise ValueError(f"{what}: the ORF factors must be [n_orf, {P}, {P}], got {A.shape}")
        if not 1 <= len(A) <= CLNL_MAX_ORF:
            raise ValueError(f"{what}: {len(A)} ORFs outside [1, {CLNL_MAX_ORF}]")
        return out + (np.ascontiguousarray(A),)

    def batch_set_clnl(self, n_modes, f, idx, freqf, phi, target, phi_grid, A, masks=None, M=None, ncol_psr=None,
                       weights=None, rcond=None):
        """The correlated likelihood grid of the batch layout (fpta_batch_set_clnl): batch_set_lnl's arguments and the
        ORF factors A [n_orf, P, P] (A A^T = Gamma). n_modes None or empty clears it. Returns (kept columns of M [P],
        ld [n_orf, G])."""
        info = self.batch_info()
        P, n = info["n_psr"], info["n_toa"]
        rank = np.zeros(P, dtype=np.int32)
        if P == 0 or n_modes is None or len(n_modes) == 0:  # without a layout: the library's own state error
            self._check(_lib.fpta_batch_set_clnl(self._h, 0, None, None, 1, None, None, None, None, 0, 0, None, None,
                                                 None, 0.0, 0, None, 0, None, _ptr(rank), None), "fpta_batch_set_clnl")
            return rank, np.zeros((0, 0))
        n_modes, f, idx, freqf, common, phi, mask, target, phi_grid, A = self._clnl_args(
            "batch_set_clnl", P, n, n_modes, f, idx, freqf, phi, masks, target, phi_grid, A)
        M, ncol_psr, weights, rcond = self._tm_args("batch_set_clnl", P, n, M, ncol_psr, weights, rcond)
        ld = np.zeros((len(A), len(phi_grid)))
        self._check(_lib.fpta_batch_set_clnl(self._h, len(n_modes), _ptr(n_modes), _ptr(f), int(common), _ptr(idx),
                                             _ptr(freqf), _ptr(phi), _ptr(mask), target, M.shape[1], _ptr(M),
                                             _ptr(ncol_psr), _ptr(weights), rcond, len(phi_grid), _ptr(phi_grid),
                                             len(A), _ptr(A), _ptr(rank), _ptr(ld)), "fpta_batch_set_clnl")
        return rank, ld

    def batch_clnl_info(self):
        """K, G and n_orf of the correlated likelihood grid that is set (0: none) and the realizations of the last
        result (fpta_batch_clnl_info)."""
        return dict(zip(("K", "G", "n_orf", "n_real"), self._info4(_lib.fpta_batch_clnl_info, "fpta_batch_clnl_info")))

    def batch_clnl(self, quadratic=False, mixed=False, coefficients=False):
        """The correlated likelihood grid of the last block (fpta_batch_clnl): (dlnL [n_orf, G, R], q [n_orf, G, R] or
        None, V [n_orf, P K, R] or None, X [P, K, R] or None). The buffers are sized from the library's own K, G and
        n_orf."""
        have, R = self.batch_clnl_info(), self._block_real()
        P = self.batch_info()["n_psr"]
        d = np.empty((have["n_orf"], have["G"], R))
        q = np.empty((have["n_orf"], have["G"], R)) if quadratic else None
        V = np.empty((have["n_orf"], P * have["K"], R)) if mixed else None
        X = np.empty((P, have["K"], R)) if coefficients else None
        self._check(_lib.fpta_batch_clnl(self._h, _ptr(d), _ptr(q), _ptr(V), _ptr(X)), "fpta_batch_clnl")
        return d, q, V, X

    def clnl_grid(self, offs, toas, nu, n_modes, f, idx, freqf, phi, target, phi_grid, A, res, masks=None, M=None,
                  ncol_psr=None, weights=None, rcond=None, tables=False):
        """The correlated likelihood grid of every row of res [n_vec, n_toa] or [n_toa] for any array (fpta_clnl_grid).
        Returns (dlnL [n_orf, G, n_vec], q [n_orf, G, n_vec], V [n_orf, P K, n_vec], X [P, K, n_vec], kept columns of M
        [P], ld [n_orf, G], T [n_orf, P K, P K] (the plan's fp64 T) or None)."""
        offs, toas, nu, res, P, n, n_vec = self._oneshot_args("clnl_grid", offs, toas, nu, res)
        n_modes, f, idx, freqf, common, phi, mask, target, phi_grid, A = self._clnl_args(
            "clnl_grid", P, n, n_modes, f, idx, freqf, phi, masks, target, phi_grid, A)
        M, ncol_psr, weights, rcond = self._tm_args("clnl_grid", P, n, M, ncol_psr, weights, rcond)
        K, G, J = 2 * int(n_modes[target]), len(phi_grid), len(A)
        d, q = np.zeros((J, G, n_vec)), np.zeros((J, G, n_vec))
        V, X = np.zeros((J, P * K, n_vec)), np.zeros((P, K, n_vec))
        rank, ld = np.zeros(P, dtype=np.int32), np.zeros((J, G))
        T = np.zeros((J, P * K, P * K)) if tables else None
        self._check(_lib.fpta_clnl_grid(self._h, P, _ptr(offs), _ptr(toas), _ptr(nu), len(n_modes), _ptr(n_modes),
                                        _ptr(f), int(common), _ptr(idx), _ptr(freqf), _ptr(phi), _ptr(mask), target,
                                        M.shape[1], _ptr(M), _ptr(ncol_psr), _ptr(weights), rcond, G, _ptr(phi_grid),
                                        J, _ptr(A), n_vec, _ptr(res), _ptr(d), _ptr(q), _ptr(V), _ptr(X), _ptr(rank),
                                        _ptr(ld), _ptr(T)), "fpta_clnl_grid")
        return d, q, V, X, rank, ld, T

    @classmethod
    def _fe_args(cls, what, P, n, n_modes, f, idx, freqf, phi, masks, fgw, sky, pos):
        """The tables of an F-statistic call: the noise model as _noise_args makes it (up to FE_MAX_COMP components;
        none: n_modes None or empty), fgw [G], sky [n_sky, 2] = (cos_gwtheta, gwphi) and pos [P, 3] within the library's
        limits."""
        if n_modes is None or len(n_modes) == 0:
            n_modes, f, idx, freqf, common, phi, mask = np.zeros(0, dtype=np.int32), None, None, None, True, None, None
        else:
            if len(n_modes) > FE_MAX_COMP:
                raise ValueError(f"{what}: {len(n_modes)} components, more than {FE_MAX_COMP}")
            n_modes, f, idx, freqf, common, phi, mask = cls._noise_args(what, P, n, n_modes, f, idx, freqf, phi, masks)
        fgw = np.atleast_1d(_f64(fgw))
        if fgw.ndim != 1 or not 1 <= len(fgw) <= FE_MAX_FREQ:
            raise ValueError(f"{what}: fgw must hold 1 .. {FE_MAX_FREQ} frequencies, got shape {fgw.shape}")
        sky = _f64(sky)
        if sky.ndim != 2 or sky.shape[1] != 2 or not 1 <= len(sky) <= FE_MAX_SKY:
            raise ValueError(f"{what}: sky must be [n_sky, 2] with 1 .. {FE_MAX_SKY} directions, got {sky.shape}")
        pos = _f64(pos)
        if pos.shape != (P, 3):
            raise ValueError(f"{what}: pos must be [{P}, 3], got {pos.shape}")
        if P > FE_MAX_PSR:
            raise ValueError(f"{what}: {P} pulsars, more than {FE_MAX_PSR}")
        return n_modes, f, idx, freqf, common, phi, mask, fgw, sky, pos

    @staticmethod
    def _fe_tables(P, G, n_sky, want):
        return ((np.zeros((2 * n_sky, P)), np.zeros((n_sky, G, 10)), np.zeros((P, G, 3)), np.zeros(G, dtype=np.int32))
                if want else (None, None, None, None))

    def batch_set_fe(self, n_modes, f, idx, freqf, phi, fgw, sky, pos, masks=None, M=None, ncol_psr=None, weights=None,
                     rcond=None, rcond_fe=None, tables=False, clear=False):
        """The F-statistics of the batch layout (fpta_batch_set_fe): the noise model as batch_set_os takes it (without a
        target), the frequencies fgw [G], the directions sky [n_sky, 2] = (cos_gwtheta, gwphi) and the pulsars' unit
        vectors pos [P, 3]. clear=True clears it. Returns (kept columns of M [P], dict(F [2 n_sky, P], Minv [n_sky, G,
        10], minv [P, G, 3], n_eff [G]) or None without tables)."""
        info = self.batch_info()
        P, n = info["n_psr"], info["n_toa"]
        rank = np.zeros(P, dtype=np.int32)
        if P == 0 or clear:  # without a layout: the library's own state error
            self._check(_lib.fpta_batch_set_fe(self._h, 0, None, None, 1, None, None, None, None, 0, None, None, None,
                                               0.0, 0, None, 0, None, None, 0.0, _ptr(rank), None, None, None, None),
                        "fpta_batch_set_fe")
            return rank, None
        if n_modes is None or len(n_modes) == 0:
            raise ValueError("batch_set_fe: the noise model needs a component (one with phi = 0 for white noise only)")
        n_modes, f, idx, freqf, common, phi, mask, fgw, sky, pos = self._fe_args(
            "batch_set_fe", P, n, n_modes, f, idx, freqf, phi, masks, fgw, sky, pos)
        M, ncol_psr, weights, rcond = self._tm_args("batch_set_fe", P, n, M, ncol_psr, weights, rcond)
        F, Minv, minv, neff = self._fe_tables(P, len(fgw), len(sky), tables)
        self._check(_lib.fpta_batch_set_fe(self._h, len(n_modes), _ptr(n_modes), _ptr(f), int(common), _ptr(idx),
                                           _ptr(freqf), _ptr(phi), _ptr(mask), M.shape[1], _ptr(M), _ptr(ncol_psr),
                                           _ptr(weights), rcond, len(fgw), _ptr(fgw), len(sky), _ptr(sky), _ptr(pos),
                                           0.0 if rcond_fe is None else float(rcond_fe), _ptr(rank), _ptr(F),
                                           _ptr(Minv), _ptr(minv), _ptr(neff)), "fpta_batch_set_fe")
        return rank, (dict(F=F, Minv=Minv, minv=minv, n_eff=neff) if tables else None)

    def batch_fe_info(self):
        """K, G and n_sky of the F-statistics that are set (0: none) and the realizations of the last result
        (fpta_batch_fe_info)."""
        return dict(zip(("K", "G", "n_sky", "n_real"), self._info4(_lib.fpta_batch_fe_info, "fpta_batch_fe_info")))

    @staticmethod
    def _fe_out(P, K, G, n_sky, R, per_frequency, full, coefficients):
        return dict(Fe_max=np.zeros(R), argmax=np.zeros((2, R), dtype=np.int32),
                    Fe_f=np.zeros((G, R)) if per_frequency else None,
                    argmax_f=np.zeros((G, R), dtype=np.int32) if per_frequency else None, Fp=np.zeros((G, R)),
                    Fe=np.zeros((n_sky, G, R)) if full else None, X=np.zeros((P, K, R)) if coefficients else None)

    def batch_fe(self, per_frequency=True, full=False, coefficients=False):
        """The F-statistics of the last block (fpta_batch_fe): a dict of Fe_max [R], argmax [2, R] (direction,
        frequency), Fe_f and argmax_f [G, R] (or None), Fp [G, R], Fe [n_sky, G, R] (the map, or None) and X [P, K, R]
        (or None). The buffers are sized from the library's own K, G and n_sky."""
        have, R = self.batch_fe_info(), self._block_real()
        o = self._fe_out(self.batch_info()["n_psr"], have["K"], have["G"], have["n_sky"], R, per_frequency, full,
                         coefficients)
        self._check(_lib.fpta_batch_fe(self._h, _ptr(o["Fe_max"]), _ptr(o["argmax"]), _ptr(o["Fe_f"]),
                                       _ptr(o["argmax_f"]), _ptr(o["Fp"]), _ptr(o["Fe"]), _ptr(o["X"])),
                    "fpta_batch_fe")
        return o

    def fe_statistic(self, offs, toas, nu, n_modes, f, idx, freqf, phi, fgw, sky, pos, res, masks=None, M=None,
                     ncol_psr=None, weights=None, rcond=None, rcond_fe=None, per_frequency=True, full=False,
                     coefficients=False, tables=False):
        """The F-statistics of every row of res [n_vec, n_toa] or [n_toa] for any array (fpta_fe_statistic). Returns
        (batch_fe's dict with R = n_vec, kept columns of M [P], batch_set_fe's tables or None)."""
        offs, toas, nu, res, P, n, n_vec = self._oneshot_args("fe_statistic", offs, toas, nu, res)
        n_modes, f, idx, freqf, common, phi, mask, fgw, sky, pos = self._fe_args(
            "fe_statistic", P, n, n_modes, f, idx, freqf, phi, masks, fgw, sky, pos)
        M, ncol_psr, weights, rcond = self._tm_args("fe_statistic", P, n, M, ncol_psr, weights, rcond)
        G, S = len(fgw), len(sky)
        o = self._fe_out(P, 2 * G, G, S, n_vec, per_frequency, full, coefficients)
        rank = np.zeros(P, dtype=np.int32)
        F, Minv, minv, neff = self._fe_tables(P, G, S, tables)
        self._check(_lib.fpta_fe_statistic(self._h, P, _ptr(offs), _ptr(toas), _ptr(nu), len(n_modes), _ptr(n_modes),
                                           _ptr(f), int(common), _ptr(idx), _ptr(freqf), _ptr(phi), _ptr(mask),
                                           M.shape[1], _ptr(M), _ptr(ncol_psr), _ptr(weights), rcond, G, _ptr(fgw), S,
                                           _ptr(sky), _ptr(pos), 0.0 if rcond_fe is None else float(rcond_fe), n_vec,
                                           _ptr(res), _ptr(o["Fe_max"]), _ptr(o["argmax"]), _ptr(o["Fe_f"]),
                                           _ptr(o["argmax_f"]), _ptr(o["Fp"]), _ptr(o["Fe"]), _ptr(o["X"]), _ptr(rank),
                                           _ptr(F), _ptr(Minv), _ptr(minv), _ptr(neff)), "fpta_fe_statistic")
        return o, rank, (dict(F=F, Minv=Minv, minv=minv, n_eff=neff) if tables else None)

    def batch_clear(self):
        self._check(_lib.fpta_batch_clear_signals(self._h), "fpta_batch_clear_signals")

    def batch_info(self):
        info = np.zeros(5, dtype=np.int64)
        self._check(_lib.fpta_batch_info(self._h, _ptr(info)), "fpta_batch_info")
        return dict(n_psr=int(info[0]), n_toa=int(info[1]), n_seg=int(info[2]), K=int(info[3]), max_np=int(info[4]))

    def batch_grid_info(self):
        """Gridded-path plan figures, the path of the last batch and why it was not the gridded path
        (fpta_batch_grid_info_n, fpta_batch_path_reason)."""
        g = np.zeros(19, dtype=np.float64)
        self._check(_lib.fpta_batch_grid_info_n(self._h, _ptr(g), len(g)), "fpta_batch_grid_info_n")
        keys = ("last_path", "ok", "n_chunks", "fma_dft", "fma_interp", "fma_direct", "grid_vals", "weight_bytes",
                "grid_mfma", "err_bound", "width", "sigma", "grid_signals", "signals", "band_rows_per_chunk")
        # slot 16: the interpolation FMAs per realization as the last block's kernel ran them (half-chunk bands)
        fma_run = float(g[16])
        d = dict(zip(keys, g.tolist()))
        d["last_path"] = int(d["last_path"])
        d["ok"] = bool(d["ok"])
        d["grid_mfma"] = int(d["grid_mfma"])
        d["width"] = int(d["width"])
        d["grid_signals"] = int(d["grid_signals"])
        d["signals"] = int(d["signals"])
        d["path_reason"] = _lib.fpta_batch_path_reason(self._h).decode()
        d["interp_kernel"] = interp_kernel_name(int(g[15]))
        d["fma_interp_run"] = fma_run if fma_run > 0 else d["fma_interp"]
        # slots 17, 18: the last block's kernel made the next block's common-signal mix / the last block took its mix
        # from the previous block's kernel (FPTA_OPT_FUSED_NEXT_MIX)
        d["next_mix_made"] = bool(g[17])
        d["next_mix_used"] = bool(g[18])
        return d

    def batch_synth(self, seed, real0, n_real, to_host=True, coeffs=False):
        info = self.batch_info()
        out = np.empty((n_real, info["n_toa"])) if to_host else None
        co = np.empty((info["n_psr"], info["K"], n_real)) if coeffs else None
        self._check(_lib.fpta_batch_synth(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(real0), int(n_real), _ptr(out),
                                          _ptr(co)), "fpta_batch_synth")
        return (out, co) if coeffs else out

    def batch_synth_spectra(self, seed, real0, n_real, seg, form, per_pulsar, tables, to_host=True, coeffs=False):
        """batch_synth with a spectrum per realization: table t (a float64 array whose first axis is the realization)
        gives signal seg[t] its amplitudes (form[t] 0) or power-law parameters (form[t] 1), per_pulsar[t] 1 with a
        pulsar axis; fakepta_amd.spectra.spectrum_tables makes the four lists. No tables: batch_synth."""
        info = self.batch_info()
        out = np.empty((n_real, info["n_toa"])) if to_host else None
        co = np.empty((info["n_psr"], info["K"], n_real)) if coeffs else None
        tables = [_f64(t) for t in tables]
        n = len(tables)
        if not (len(seg) == len(form) == len(per_pulsar) == n):
            raise ValueError("batch_synth_spectra: seg, form, per_pulsar and tables must have one entry per table")
        seg, form, per = (np.ascontiguousarray(v, dtype=np.int32).reshape(n) for v in (seg, form, per_pulsar))
        rows = np.array([t.shape[0] if t.ndim else 0 for t in tables], dtype=np.int32)
        ptrs = (_vp * max(n, 1))(*[t.ctypes.data for t in tables])
        self._check(_lib.fpta_batch_synth_spectra(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(real0), int(n_real), n,
                                                  _ptr(seg), _ptr(form), _ptr(per), _ptr(rows),
                                                  ctypes.cast(ptrs, _vp), _ptr(out), _ptr(co)),
                    "fpta_batch_synth_spectra")
        return (out, co) if coeffs else out

    def batch_synth_from_z(self, z):
        z = _f64(z)
        info = self.batch_info()
        n_real = z.shape[0]
        assert z.ndim == 5 and z.shape[1:3] == (info["n_seg"], info["n_psr"]) and z.shape[4] == 2
        out = np.empty((n_real, info["n_toa"]))
        self._check(_lib.fpta_batch_synth_from_z(self._h, n_real, z.shape[3], _ptr(z), _ptr(out)),
                    "fpta_batch_synth_from_z")
        return out

    def batch_download(self, r_begin, r_count):
        """Realizations [r_begin, r_begin + r_count) of the last block -> host [r_count, n_toa]."""
        _, ld, _ = self.batch_device_out()
        out = np.empty((r_count, ld))
        self._check(_lib.fpta_batch_download(self._h, int(r_begin), int(r_count), _ptr(out)), "fpta_batch_download")
        return out

    def batch_device_out(self):
        p, ld, nr = _vp(), _i64(), _i32()
        self._check(_lib.fpta_batch_device_out(self._h, ctypes.byref(p), ctypes.byref(ld), ctypes.byref(nr)),
                    "fpta_batch_device_out")
        return p.value, ld.value, nr.value

    def batch_correlations(self, mode=2):
        """0: [R, P, P] per realization; 1: [P, P] sum; 2: [P, P] sum of normalized; 3: [R, P] autos."""
        info = self.batch_info()
        _, _, R = self.batch_device_out()
        P = info["n_psr"]
        shape = {0: (R, P, P), 1: (P, P), 2: (P, P), 3: (R, P)}[mode]
        out = np.empty(shape)
        self._check(_lib.fpta_batch_correlations(self._h, int(mode), _ptr(out)), "fpta_batch_correlations")
        return out

    def batch_checksums(self):
        _, _, nr = self.batch_device_out()
        s = np.empty((nr, 2))
        self._check(_lib.fpta_batch_checksums(self._h, _ptr(s)), "fpta_batch_checksums")
        return s

    def batch_synth_checksums(self, seed, real0, n_real, batch=4096):
        """Realizations real0 .. real0 + n_real - 1 streamed in batches of <= batch with no host round trip in
        between; returns their checksums [n_real, 2] (fpta_batch_synth_checksums)."""
        out = np.empty((int(n_real), 2))
        self._check(_lib.fpta_batch_synth_checksums(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(real0), int(n_real),
                                                    int(batch), _ptr(out)), "fpta_batch_synth_checksums")
        return out

    # --------------------------------------------------------------- tuning / profiling
    def set_option(self, key, value):
        self._check(_lib.fpta_set_option(self._h, int(key), int(value)), "fpta_set_option")

    def get_option(self, key):
        v = _i64()
        self._check(_lib.fpta_get_option(self._h, int(key), ctypes.byref(v)), "fpta_get_option")
        return int(v.value)

    def options(self):
        """Snapshot of every option (restore with set_options)."""
        return {k: self.get_option(k) for k in OPTIONS}

    def set_options(self, opts):
        for k, v in opts.items():
            self.set_option(k, v)

    def kernel_stats(self, which):
        n, ms = _i64(), _dbl()
        self._check(_lib.fpta_kernel_stats(self._h, int(which), ctypes.byref(n), ctypes.byref(ms)),
                    "fpta_kernel_stats")
        return n.value, ms.value

    def reset_stats(self):
        self._check(_lib.fpta_reset_stats(self._h), "fpta_reset_stats")

    def synchronize(self):
        self._check(_lib.fpta_synchronize(self._h), "fpta_synchronize")

    def debug_fill_out(self, value):
        """Fill the last device block with `value` (tests: the next batch must overwrite every sample)."""
        self._check(_lib.fpta_debug_fill_out(self._h, float(value)), "fpta_debug_fill_out")

    def debug_fused_shape(self):
        """The variant of the reported k_grid_fused instance the last gridded block ran: 1 / 2 the instance of the
        layout's draw shape (csrc/fused_sched.h), 0 the fallback, -1 no k_grid_fused."""
        shape = np.zeros(1, dtype=np.int32)
        self._check(_lib.fpta_debug_fused_shape(self._h, _ptr(shape)), "fpta_debug_fused_shape")
        return int(shape[0])

    def debug_philox(self, ctr, key):
        ctr = np.ascontiguousarray(ctr, dtype=np.uint32).reshape(-1, 4)
        key = np.ascontiguousarray(key, dtype=np.uint32)
        out = np.empty_like(ctr)
        self._check(_lib.fpta_debug_philox(self._h, len(ctr), _ptr(ctr), _ptr(key), _ptr(out)), "fpta_debug_philox")
        return out

    def debug_normals(self, words):
        """philox.h normals4 on the device for uint32 words [n, 4] -> float64 [n, 4] (oracle normals4)."""
        words = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, 4)
        out = np.empty(words.shape, dtype=np.float64)
        self._check(_lib.fpta_debug_normals(self._h, len(words), _ptr(words), _ptr(out)), "fpta_debug_normals")
        return out


class _Borrowed(Context):
    """A device context owned by a MultiContext (not destroyed by this wrapper). It keeps its parent alive and is
    invalidated when the parent closes, so a call on it never reaches a context fpta_multi_destroy has freed."""

    def __init__(self, handle, device, parent):
        self._h = handle
        self.device = device
        self._parent = parent

    def close(self):
        self._h = None

    def __getattribute__(self, name):
        if name not in ("_h", "_parent", "device", "close", "__class__", "__dict__") and not name.startswith("__"):
            parent = object.__getattribute__(self, "_parent")
            if object.__getattribute__(self, "_h") is None or getattr(parent, "_h", None) is None:
                raise FptaError("context of a closed MultiContext")
        return object.__getattribute__(self, name)


class MultiContext:
    """Several devices driven from one process (fpta_multi_*): the layout is replicated on each device,
    realizations are sharded contiguously over them and only per-realization checksums come back."""

    def __init__(self, devices):
        devs = np.ascontiguousarray(devices, dtype=np.int32)
        h = _vp()
        rc = _lib.fpta_multi_create(len(devs), _ptr(devs), ctypes.byref(h))
        if rc != 0:
            raise FptaError(f"fpta_multi_create({list(devs)}) failed ({rc}): {_lib.fpta_last_error(None).decode()}")
        self._h = h
        self.devices = [int(d) for d in devs]

    def _check(self, rc, what):
        if rc < 0:
            raise FptaError(f"{what} failed ({rc}): {_lib.fpta_multi_last_error(self._h).decode()}")
        return rc

    def close(self):
        if getattr(self, "_h", None):
            for b in getattr(self, "_borrowed", ()):
                b.close()
            _lib.fpta_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return int(_lib.fpta_multi_size(self._h))

    def context(self, i):
        if not getattr(self, "_h", None):
            raise FptaError("MultiContext is closed")
        b = _Borrowed(_lib.fpta_multi_context(self._h, int(i)), self.devices[i], self)
        self.__dict__.setdefault("_borrowed", []).append(b)
        return b

    def set_toas(self, offs, toas, nu):
        offs = np.ascontiguousarray(offs, dtype=np.int64)
        toas, nu = _f64(toas), _f64(nu)
        self._check(_lib.fpta_multi_set_toas(self._h, len(offs) - 1, _ptr(offs), _ptr(toas), _ptr(nu)),
                    "fpta_multi_set_toas")

    def add_signal(self, kind, f, amp, idx=0.0, freqf=1400.0, L=None, mask=None):
        f, amp = _f64(f), _f64(amp)
        L = None if L is None else _f64(L)
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        return self._check(_lib.fpta_multi_add_signal(self._h, int(kind), f.shape[-1], _ptr(f), _ptr(amp),
                                                      float(idx), float(freqf), _ptr(L), _ptr(m)),
                           "fpta_multi_add_signal")

    def set_white(self, sigma=None, blocks=None, ecorr_sigma=None):
        s = None if sigma is None else _f64(sigma)
        nb, bo, bi, es = 0, None, None, None
        if blocks:
            nb = len(blocks)
            bo = np.concatenate([[0], np.cumsum([len(b) for b in blocks])]).astype(np.int64)
            bi = np.concatenate([np.asarray(b, dtype=np.int64) for b in blocks]).astype(np.int64)
            es = _f64(ecorr_sigma)
        self._check(_lib.fpta_multi_set_white(self._h, _ptr(s), nb, _ptr(bo), _ptr(bi), _ptr(es)),
                    "fpta_multi_set_white")

    def set_option(self, key, value):
        self._check(_lib.fpta_multi_set_option(self._h, int(key), int(value)), "fpta_multi_set_option")

    def set_gather(self, mode):
        """GATHER_AUTO (RCCL when the devices are distinct), GATHER_RCCL or GATHER_HOST (fpta_multi_set_gather)."""
        self._check(_lib.fpta_multi_set_gather(self._h, int(mode)), "fpta_multi_set_gather")

    def last_gather(self):
        """The route the last synth_checksums took: GATHER_RCCL or GATHER_HOST (0 before any)."""
        return int(_lib.fpta_multi_last_gather(self._h))

    def synth_checksums(self, seed, real0, n_real, batch=4096):
        """Per-realization (sum, sum of squares) of realizations real0 .. real0 + n_real - 1: [n_real, 2]."""
        out = np.empty((int(n_real), 2))
        self._check(_lib.fpta_multi_synth(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(real0), int(n_real),
                                          int(batch), _ptr(out)), "fpta_multi_synth")
        return out


class Comm:
    """RCCL communicator of one rank on one context (fpta_comm_*): the library's own RCCL on the kernels' HIP
    runtime. Rank 0 makes the unique id (Comm.unique_id()); every rank passes it to Comm(ctx, nranks, rank, uid)."""

    @staticmethod
    def unique_id():
        buf = ctypes.create_string_buffer(COMM_ID_BYTES)
        rc = _lib.fpta_comm_unique_id(ctypes.cast(buf, _vp))
        if rc != 0:
            raise FptaError(f"fpta_comm_unique_id failed ({rc}): {_lib.fpta_last_error(None).decode()}")
        return buf.raw

    def __init__(self, ctx, nranks, rank, uid):
        if len(uid) != COMM_ID_BYTES:
            raise ValueError(f"RCCL unique id must be {COMM_ID_BYTES} bytes")
        buf = ctypes.create_string_buffer(bytes(uid), COMM_ID_BYTES)
        h = _vp()
        rc = _lib.fpta_comm_init_rank(ctx._h, int(nranks), int(rank), ctypes.cast(buf, _vp), ctypes.byref(h))
        if rc != 0:
            raise FptaError(f"fpta_comm_init_rank(nranks={nranks}, rank={rank}) failed ({rc}): "
                            f"{_lib.fpta_last_error(ctx._h).decode()}")
        self._h = h
        self.ctx = ctx  # the communicator runs on ctx's device and stream: keep it alive
        self.nranks, self.rank = int(nranks), int(rank)

    def _check(self, rc, what):
        if rc != 0:
            raise FptaError(f"{what} failed ({rc}): {_lib.fpta_comm_last_error(self._h).decode()}")

    def max(self, x):
        v = _dbl(float(x))
        self._check(_lib.fpta_comm_max(self._h, ctypes.byref(v)), "fpta_comm_max")
        return float(v.value)

    def gather(self, arr):
        """Rank 0: every rank's float64 `arr` (same shape on every rank) stacked in rank order; others: None."""
        a = _f64(arr)
        out = np.empty((self.nranks,) + a.shape) if self.rank == 0 else None
        self._check(_lib.fpta_comm_gather(self._h, _ptr(a), a.size, _ptr(out)), "fpta_comm_gather")
        return out

    def close(self):
        if getattr(self, "_h", None):
            _lib.fpta_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default = {}
_lock = threading.Lock()


def default_device():
    return int(os.environ.get("FAKEPTA_AMD_DEVICE", os.environ.get("LOCAL_RANK", "0")))


def get_context(device=None):
    """Process-wide context for the drop-in Pulsar methods (created on first use)."""
    dev = default_device() if device is None else int(device)
    with _lock:
        ctx = _default.get(dev)
        if ctx is None:
            ctx = Context(dev)
            _default[dev] = ctx
        return ctx


def device_count():
    n = _c_int()
    rc = _lib.fpta_device_count(ctypes.byref(n))
    return n.value if rc == 0 else 0
