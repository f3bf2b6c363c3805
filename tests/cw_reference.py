"""Reference evaluations of the continuous-wave delay that Pulsar.add_cgw injects (enterprise_extensions'
cw_delay with evolve=True, tref=0, p_phase=None, p_dist=1), restated from its definition:

  cw_delay_numpy   the literal fp64 numpy evaluation, term by term as the definition is written (its phase line
                   subtracts two terms of up to ~1e7 rad: it is the yardstick of what fp64 achieves, not a target)
  cw_delay_mp      the same definition in mpmath at 60 digits, rounded to fp64 at the end: the truth of the fixture
                   tests/golden/g10_cw.npz (tools/gen_cw_golden.py)

Both take the fp64 inputs exactly as given. Sources are rows of COLUMNS, the layout of fpta_cw_accumulate."""
import numpy as np

from fakepta import constants as const
from fakepta.correlated_noises import create_gw_antenna_pattern

COLUMNS = ("cos_gwtheta", "gwphi", "cos_inc", "log10_mc", "log10_fgw", "log10_h", "phase0", "psi", "psrterm")


def cw_delay_numpy(toas, pos, pdist, cos_gwtheta, gwphi, cos_inc, log10_mc, log10_fgw, log10_h, phase0, psi,
                   psrterm, p_dist=1.0):
    toas = np.asarray(toas, dtype=float)
    mc = 10 ** log10_mc * const.Tsun
    w0 = np.pi * 10 ** log10_fgw
    gwtheta = np.arccos(cos_gwtheta)
    inc = np.arccos(cos_inc)
    dist = 2 * mc ** (5 / 3) * w0 ** (2 / 3) / 10 ** log10_h
    L = (pdist[0] + pdist[1] * p_dist) * const.kpc / const.c
    fplus, fcross, cosMu = create_gw_antenna_pattern(np.asarray(pos, float), np.array([gwtheta]), np.array([gwphi]))
    fplus, fcross, cosMu = fplus[0], fcross[0], cosMu[0]
    tp = toas - L * (1 - cosMu)
    K = 256 / 5 * mc ** (5 / 3) * w0 ** (8 / 3)

    def r(x):
        omega = w0 * (1 - K * x) ** (-3 / 8)
        phase = phase0 / 2 + (w0 ** (-5 / 3) - omega ** (-5 / 3)) / (32 * mc ** (5 / 3))
        alpha = mc ** (5 / 3) / (dist * omega ** (1 / 3))
        A = -0.5 * np.sin(2 * phase) * (3 + np.cos(2 * inc))
        B = 2 * np.cos(2 * phase) * np.cos(inc)
        rplus = alpha * (-A * np.cos(2 * psi) + B * np.sin(2 * psi))
        rcross = alpha * (A * np.sin(2 * psi) + B * np.cos(2 * psi))
        return rplus, rcross

    rp, rc = r(toas)
    if psrterm:
        rp_p, rc_p = r(tp)
        return fplus * (rp_p - rp) + fcross * (rc_p - rc)
    return -fplus * rp - fcross * rc


def cw_delay_mp(toas, pos, pdist, cos_gwtheta, gwphi, cos_inc, log10_mc, log10_fgw, log10_h, phase0, psi, psrterm,
                p_dist=1.0, dps=60):
    import mpmath as mp

    with mp.workdps(dps):
        f = mp.mpf
        Tsun = f(const.GMsun) / f(const.c) ** 3
        mc = f(10) ** f(float(log10_mc)) * Tsun
        w0 = mp.pi * f(10) ** f(float(log10_fgw))
        h = f(10) ** f(float(log10_h))
        cth, ci = f(float(cos_gwtheta)), f(float(cos_inc))
        sth = mp.sqrt(1 - cth * cth)            # sin(arccos(cos_gwtheta))
        cph, sph = mp.cos(f(float(gwphi))), mp.sin(f(float(gwphi)))
        c2i = 2 * ci * ci - 1                   # cos(2 arccos(cos_inc))
        c2p, s2p = mp.cos(2 * f(float(psi))), mp.sin(2 * f(float(psi)))
        dist = 2 * mc ** (f(5) / 3) * w0 ** (f(2) / 3) / h
        L = (f(float(pdist[0])) + f(float(pdist[1])) * f(float(p_dist))) * f(const.kpc) / f(const.c)
        px, py, pz = (f(float(x)) for x in pos)
        mpos = sph * px - cph * py
        npos = -cth * cph * px - cth * sph * py + sth * pz
        opos = -sth * cph * px - sth * sph * py - cth * pz
        fplus = (mpos ** 2 - npos ** 2) / (2 * (1 + opos))
        fcross = mpos * npos / (1 + opos)
        cosMu = -opos
        K = f(256) / 5 * mc ** (f(5) / 3) * w0 ** (f(8) / 3)
        hp0 = f(float(phase0)) / 2

        def r(x):
            omega = w0 * (1 - K * x) ** (-f(3) / 8)
            phase = hp0 + (w0 ** (-f(5) / 3) - omega ** (-f(5) / 3)) / (32 * mc ** (f(5) / 3))
            alpha = mc ** (f(5) / 3) / (dist * omega ** (f(1) / 3))
            A = -mp.sin(2 * phase) * (3 + c2i) / 2
            B = 2 * mp.cos(2 * phase) * ci
            return alpha * (-A * c2p + B * s2p), alpha * (A * s2p + B * c2p)

        out = np.empty(len(toas))
        for i, t in enumerate(np.asarray(toas, dtype=float)):
            t = f(float(t))
            rp, rc = r(t)
            if psrterm:
                rp_p, rc_p = r(t - L * (1 - cosMu))
                out[i] = float(fplus * (rp_p - rp) + fcross * (rc_p - rc))
            else:
                out[i] = float(-fplus * rp - fcross * rc)
        return out
