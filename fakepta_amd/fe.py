"""Continuous-wave F-statistics: per realization the Earth-term Fe-statistic of a circular binary on a grid of sky
directions and frequencies and the incoherent Fp-statistic per frequency, computed on the device (fpta_batch_set_fe,
fpta_batch_fe, fpta_fe_statistic; the definition is in include/fakepta_amd.h). The device returns Fe_max [R] with its
(direction, frequency), Fe_f [G, R] = max over the directions with its argmax, Fp [G, R] and on request the whole map
Fe [n_sky, G, R]. The helpers here build the sky grid and hold the host algebra around them: the false-alarm
probability of one Fe value and the maximum-likelihood direction and frequency. BatchSimulator.set_fe_statistic /
fe_statistic and the drop-in fake_pta.fe_statistic_array share them; the layout-to-components code is fakepta_amd.os's
and the keyword names are fakepta_amd.cw's. Nothing here needs a device except statistic_array's one call."""
import numpy as np

from . import _capi
from . import os as _os
from . import tm as _tm

MAX_COMP, MAX_FREQ, MAX_SKY, MAX_PSR = _capi.FE_MAX_COMP, _capi.FE_MAX_FREQ, _capi.FE_MAX_SKY, _capi.FE_MAX_PSR


def sky_grid(nside=None, sky=None):
    """[n_sky, 2] rows of (cos_gwtheta, gwphi): the pixel centres of a HEALPix RING map of `nside`, or the explicit
    array `sky`; ValueError when both or neither are given, or a direction is off the sphere."""
    if (nside is None) == (sky is None):
        raise ValueError("the sky grid takes either nside or sky [n, 2] of (cos_gwtheta, gwphi)")
    if nside is not None:
        if int(nside) != nside or int(nside) < 1 or 12 * int(nside) ** 2 > MAX_SKY:
            raise ValueError(f"nside {nside!r}: 12 nside^2 must be 12 .. {MAX_SKY} directions")
        from .orf import pix2ang_ring
        theta, phi = pix2ang_ring(int(nside))
        return np.ascontiguousarray(np.stack([np.cos(theta), phi], axis=1))
    sky = np.asarray(sky, dtype=np.float64)
    if sky.ndim == 1 and sky.shape == (2,):
        sky = sky[None]
    if sky.ndim != 2 or sky.shape[1] != 2 or not 1 <= len(sky) <= MAX_SKY:
        raise ValueError(f"sky must be [n, 2] with 1 .. {MAX_SKY} directions, got shape {sky.shape}")
    bad = np.argwhere(~((sky[:, 0] >= -1) & (sky[:, 0] <= 1) & np.isfinite(sky[:, 1])))
    if len(bad):
        raise ValueError(f"direction {bad[0][0]}: cos_gwtheta outside [-1, 1] or gwphi not finite")
    return np.ascontiguousarray(sky)


def check_frequencies(fgw):
    """fgw as [G] float64: positive and finite, 1 <= G <= MAX_FREQ, else ValueError naming the frequency."""
    fgw = np.atleast_1d(np.asarray(fgw, dtype=np.float64))
    if fgw.ndim != 1 or not 1 <= len(fgw) <= MAX_FREQ:
        raise ValueError(f"fgw must hold 1 .. {MAX_FREQ} frequencies, got shape {fgw.shape}")
    bad = np.argwhere(~(np.isfinite(fgw) & (fgw > 0)))
    if len(bad):
        raise ValueError(f"frequency {bad[0][0]}: not positive and finite")
    return np.ascontiguousarray(fgw)


def positions_of(psrs, what):
    """[P, 3] unit vectors of the pulsars; ValueError when one has no pos."""
    try:
        return np.array([np.asarray(p.pos, dtype=np.float64) for p in psrs]).reshape(len(psrs), 3)
    except AttributeError as e:
        raise ValueError(f"{what}: every pulsar needs pos ({e})") from None


def model_of(segments, n_psr):
    """os.noise_model of the segments, within MAX_COMP components. A model without a Gaussian process (white noise only)
    is one achromatic component of one mode at 1e-8 Hz with phi = 0: the library leaves a mode with phi = 0 out of the
    model, so the tables are those of no component at all, and the batch call (where no component means "clear") and
    the one-shot call take the same model."""
    segments = list(segments)
    if not segments:
        return dict(names=[], n_modes=np.ones(1, dtype=np.int32), f=np.full(1, 1e-8), idx=np.zeros(1),
                    freqf=np.full(1, 1400.0), phi=np.zeros((n_psr, 1)), masks=None)
    model = _os.noise_model(segments, n_psr)
    if len(model["n_modes"]) > MAX_COMP:
        raise ValueError(f"the noise model has {len(model['n_modes'])} components, more than {MAX_COMP}")
    return model


def false_alarm(Fe):
    """exp(-Fe) (1 + Fe): the probability that 2 Fe, chi^2 with 4 degrees of freedom under the null, exceeds the value
    at one (direction, frequency). NaN stays NaN."""
    Fe = np.asarray(Fe, dtype=np.float64)
    return np.exp(-Fe) * (1.0 + Fe)


def derive(out, fgw, sky):
    """batch_fe's dict plus what the host derives: cos_gwtheta_ml, gwphi_ml, fgw_ml [R] of the overall maximum (NaN
    where every point is singular), fap_max [R] = false_alarm(Fe_max) (of one trial, not of the maximum), and the grids
    fgw and sky."""
    fgw, sky = np.asarray(fgw, dtype=np.float64), np.asarray(sky, dtype=np.float64)
    out = dict(out)
    s, g = out["argmax"][0], out["argmax"][1]
    ok = (s >= 0) & (g >= 0)
    out["cos_gwtheta_ml"] = np.where(ok, sky[np.where(ok, s, 0), 0], np.nan)
    out["gwphi_ml"] = np.where(ok, sky[np.where(ok, s, 0), 1], np.nan)
    out["fgw_ml"] = np.where(ok, fgw[np.where(ok, g, 0)], np.nan)
    out["fap_max"] = false_alarm(out["Fe_max"])
    out["fgw"], out["sky"] = fgw, sky
    return out


def statistic_array(psrs, fgw, nside=None, sky=None, signals=None, Mmats="tm", weights="white", rcond=None,
                    rcond_fe=None, per_frequency=True, full=False, ctx=None):
    """The F-statistics of psr.residuals for a whole array in one device call (fpta_fe_statistic): the dict of derive()
    for one residual vector (R = 1). The noise model is what the pulsars carry: signal_model (every GP, or `signals`;
    a common process enters as each pulsar's auto-term) and the white noise of the noisedict as weights. ECORR is not
    part of the weights."""
    fgw, sky = check_frequencies(fgw), sky_grid(nside, sky)
    segs = _os.segments_of(psrs, signals)
    model = model_of(segs, len(psrs))
    M, ncol = _os.design_of(psrs, Mmats, "fe_statistic_array")
    offs = np.concatenate([[0], np.cumsum([len(p.toas) for p in psrs])]).astype(np.int64)
    toas = np.concatenate([np.asarray(p.toas, dtype=np.float64) for p in psrs])
    nu = np.concatenate([np.asarray(p.freqs, dtype=np.float64) for p in psrs])
    res = np.concatenate([np.asarray(p.residuals, dtype=np.float64) for p in psrs])
    ctx = ctx if ctx is not None else _capi.get_context()
    out, _, _ = ctx.fe_statistic(offs, toas, nu, model["n_modes"], model["f"], model["idx"], model["freqf"],
                                 model["phi"], fgw, sky, positions_of(psrs, "fe_statistic_array"), res,
                                 masks=model["masks"], M=M, ncol_psr=ncol,
                                 weights=_tm.weights_of(psrs, weights, int(offs[-1])), rcond=rcond, rcond_fe=rcond_fe,
                                 per_frequency=per_frequency, full=full)
    return derive(out, fgw, sky)
