"""Anisotropic overlap reduction function: HEALPix RING pixel centres and the weighted antenna-pattern Gram matrix
(libfakepta_amd: fpta_healpix_pix2ang_ring on the host, fpta_orf_anisotropic on the GPU). No healpy."""
import numpy as np

from . import _capi


def npix2nside(npix):
    """nside of a map of npix pixels; ValueError when npix is not 12 nside^2 (as healpy raises)."""
    npix = int(npix)
    nside = int(round((npix / 12.0) ** 0.5)) if npix > 0 else 0
    if nside < 1 or 12 * nside * nside != npix:
        raise ValueError(f"Wrong pixel number (it is not 12*nside**2): {npix}")
    return nside


def pix2ang_ring(nside):
    """(theta, phi) of every pixel centre of a RING-ordered map, as healpy.pix2ang(nside, arange(npix))."""
    return _capi.pix2ang_ring(nside)


def anisotropic_orf(pos, h_maps, ctx=None):
    """ORF of the pulsars at unit vectors pos [P, 3] for RING-ordered maps: a 1-D map gives [P, P], a 2-D array
    [M, npix] gives [M, P, P] from one call (the maps share the antenna patterns)."""
    h = np.asarray(h_maps, dtype=np.float64)
    if h.ndim not in (1, 2):
        raise ValueError("anisotropic_orf: h_maps must be one map or an array [M, npix] of maps")
    nside = npix2nside(h.shape[-1])
    ctx = _capi.get_context() if ctx is None else ctx
    out = ctx.orf_anisotropic(np.asarray(pos, dtype=np.float64).reshape(-1, 3), nside, np.atleast_2d(h))
    return out[0] if h.ndim == 1 else out
