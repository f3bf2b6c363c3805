"""Truth of fpta_batch_synth_spectra: oracle.batch_coefficients and oracle.batch_synth restated with the amplitude of
realization r taken from row r of a table, on top of the oracle's own normals (O.gp_normals). No GPU needed."""
import numpy as np

from oracle import fakepta_oracle as O


def coefficients(segs, P, seed, real0, n_real, amps):
    """Per signal [R, P, N, 2]. amps: {signal index: [R, N] or [R, P, N]}; other signals keep seg.amp. A row shared by
    the pulsars of a per-pulsar signal does not reach a (pulsar, mode) whose layout amplitude is 0."""
    reals, out = np.arange(real0, real0 + n_real), []
    for s, seg in enumerate(segs):
        z = np.stack([O.gp_normals(seed, reals, p, s, seg.n_modes) for p in range(P)], axis=1)
        a = np.broadcast_to(seg.amp, (n_real,) + seg.amp.shape) if s not in amps else np.asarray(amps[s], float)
        if seg.kind == 0:
            a = a if a.ndim == 3 else np.where(seg.amp[None] == 0.0, 0.0, a[:, None, :])
            out.append(a[..., None] * z)
        else:
            out.append(a[:, None, :, None] * np.einsum("pq,rqnc->rpnc", seg.L, z))
    return out


def download(coefs, P, n_real):
    """The coefficient download's layout [P][K][R] (counter_space.oracle_coeffs)."""
    a = [np.pad(x, ((0, 0), (0, 0), (0, x.shape[2] % 2), (0, 0))) for x in coefs]
    return np.concatenate([np.transpose(x, (1, 2, 3, 0)).reshape(P, -1, n_real) for x in a], axis=1)


def synth(offs, toas, freqs, segs, seed, real0, n_real, amps):
    """The GP part of O.batch_synth with per-realization amplitudes: [n_real, n_toa]."""
    P = len(offs) - 1
    out = np.zeros((n_real, offs[-1]))
    for seg, a in zip(segs, coefficients(segs, P, seed, real0, n_real, amps)):
        for p in range(P):
            sl = slice(offs[p], offs[p + 1])
            ph = np.outer(toas[sl], seg.w[p] if seg.kind == 0 else seg.w)
            ch = (seg.freqf / freqs[sl]) ** seg.idx
            out[:, sl] += ch[None, :] * (a[:, p, :, 0] @ np.cos(ph).T + a[:, p, :, 1] @ np.sin(ph).T)
    return out
