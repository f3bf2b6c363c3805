"""Per-realization spectra of a batch block, host side (no GPU): the C-ABI surface, fakepta_amd.spectra's
spectrum_tables, and the validator of csrc/spectra_host.h in a stand-alone C++ program built with the address and
undefined-behaviour sanitizers."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fakepta_amd.h")
LIB = os.path.join(ROOT, "fakepta_amd", "lib", "libfakepta_amd.so")
CSRC = os.path.join(ROOT, "fakepta_amd", "csrc")


def test_abi_declares_exports_and_binds_synth_spectra():
    import inspect
    text = open(HEADER).read()
    assert re.search(r"^int\s+fpta_batch_synth_spectra\s*\(", text, flags=re.M)
    assert re.search(r"^#define\s+FPTA_VERSION\s+10300\b", text, flags=re.M)
    assert hasattr(ctypes.CDLL(LIB), "fpta_batch_synth_spectra")
    from fakepta_amd import _capi
    assert "fpta_batch_synth_spectra" in _capi.EXPORTED
    assert callable(_capi.Context.batch_synth_spectra)
    from fakepta_amd.batch import BatchSimulator, simulate_sharded
    assert "spectra" in inspect.signature(BatchSimulator.synth).parameters
    assert "spectra" in inspect.signature(simulate_sharded).parameters


# ----------------------------------------------------------------------------- spectrum_tables
class _Sim:
    """The host copy of a layout that spectrum_tables reads: 3 pulsars; red noise of 5 modes (pulsar 1 carries 3,
    pulsar 2 none) and a common signal of 4 modes."""

    def __init__(self):
        T = 3.0e8
        self.psrs = [None] * 3
        f_rn = np.tile(np.arange(1, 6) / T, (3, 1))
        f_rn[1] *= 1.5
        a_rn = np.full((3, 5), 1e-7)
        a_rn[1, 3:] = 0.0
        a_rn[2] = 0.0
        f_gw = np.arange(1, 5) / T
        self.segments = [dict(name="red_noise", kind=0, f=f_rn, amp=a_rn, id=0),
                         dict(name="gw_common", kind=1, f=f_gw, amp=np.full(4, 1e-8), id=1)]


@pytest.fixture
def sim(monkeypatch):
    from fakepta_amd import _capi

    def no_context(*a, **k):
        raise AssertionError("a device context was requested")
    monkeypatch.setattr(_capi, "get_context", no_context)
    return _Sim()


def test_spectrum_tables_shapes_and_broadcasting(sim):
    from fakepta_amd.spectra import slice_spectra, spectrum_tables
    R, P = 4, 3
    rng = np.random.default_rng(0)
    # common signal: [N] broadcasts, [R, N] as given
    a = rng.uniform(1e-9, 1e-8, (R, 4))
    seg, form, per, tabs = spectrum_tables(sim, {"gw_common": dict(amp=a[0])}, R)
    assert (seg, form, per) == ([1], [0], [0]) and tabs[0].shape == (R, 4)
    np.testing.assert_array_equal(tabs[0], np.tile(a[0], (R, 1)))
    assert tabs[0].dtype == np.float64 and tabs[0].flags.c_contiguous
    seg, form, per, tabs = spectrum_tables(sim, {"gw_common": dict(amp=a)}, R)
    np.testing.assert_array_equal(tabs[0], a)
    # psd is in the units of signal_model[...]['psd']: amp = sqrt(psd * df)
    f = sim.segments[1]["f"]
    seg, form, per, tabs = spectrum_tables(sim, {"gw_common": dict(psd=a)}, R)
    np.testing.assert_array_equal(tabs[0], np.sqrt(a * np.diff(np.append(0.0, f))))
    # per-pulsar signal: a shared row stays [R, N] as amp and takes each pulsar's df as psd (zeros where the layout's)
    rn = rng.uniform(1e-8, 1e-7, (R, 5))
    seg, form, per, tabs = spectrum_tables(sim, {"red_noise": dict(amp=rn)}, R)
    assert (seg, form, per) == ([0], [0], [0]) and tabs[0].shape == (R, 5)
    seg, form, per, tabs = spectrum_tables(sim, {"red_noise": dict(psd=rn)}, R)
    assert per == [1] and tabs[0].shape == (R, P, 5)
    df = np.diff(np.concatenate([np.zeros((P, 1)), sim.segments[0]["f"]], axis=1), axis=1)
    want = np.sqrt(rn[:, None, :] * df)
    want[:, 1, 3:] = 0.0
    want[:, 2] = 0.0
    np.testing.assert_array_equal(tabs[0], want)
    full = np.where(sim.segments[0]["amp"] == 0.0, 0.0, rng.uniform(1e-8, 1e-7, (R, P, 5)))
    seg, form, per, tabs = spectrum_tables(sim, {"red_noise": dict(amp=full)}, R)
    assert per == [1]
    np.testing.assert_array_equal(tabs[0], full)
    # power law: scalars broadcast, [R] and [R, P] by shape and kind; both signals at once come back in id order
    lA, g = rng.uniform(-15, -13, R), rng.uniform(2, 6, (R, P))
    seg, form, per, tabs = spectrum_tables(sim, {"gw_common": dict(log10_A=lA, gamma=4.0),
                                                 "red_noise": dict(log10_A=-14.0, gamma=g)}, R)
    assert (seg, form, per) == ([0, 1], [1, 1], [1, 0])
    assert tabs[0].shape == (R, P, 2) and tabs[1].shape == (R, 2)
    np.testing.assert_array_equal(tabs[1], np.stack([lA, np.full(R, 4.0)], axis=1))
    np.testing.assert_array_equal(tabs[0][..., 0], -14.0)
    np.testing.assert_array_equal(tabs[0][..., 1], g)
    seg, form, per, tabs = spectrum_tables(sim, {0: dict(log10_A=lA, gamma=3.0)}, R)  # by id; [R] on a per-pulsar signal
    assert (seg, per) == ([0], [0]) and tabs[0].shape == (R, 2)
    assert spectrum_tables(sim, {}, R) == ([], [], [], [])
    # slicing a job's spectra per batch
    part = slice_spectra({"gw_common": dict(log10_A=lA, gamma=4.0), "red_noise": dict(amp=full), 0: dict(amp=rn[0])}, 1, 2)
    np.testing.assert_array_equal(part["gw_common"]["log10_A"], lA[1:3])
    assert part["gw_common"]["gamma"] == 4.0 and part["red_noise"]["amp"].shape == (2, P, 5)
    np.testing.assert_array_equal(part[0]["amp"], rn[0])


def test_spectrum_tables_errors(sim):
    from fakepta_amd.spectra import spectrum_tables
    R, P = 4, 3
    gw, rn = np.full((R, 4), 1e-8), np.where(sim.segments[0]["amp"] == 0.0, 0.0, np.full((R, P, 5), 1e-7))

    def put(a, idx, v):
        a = a.copy()
        a[idx] = v
        return a
    cases = [
        ({"gw_common": dict(amp=put(gw, (2, 1), np.nan))}, "spectra['gw_common']: realization 2, mode 1: non-finite amplitude"),
        ({"gw_common": dict(amp=put(gw, (3, 0), -1.0))}, "spectra['gw_common']: realization 3, mode 0: negative amplitude"),
        ({"gw_common": dict(psd=put(gw, (0, 2), -1.0))}, "realization 0, mode 2: negative psd"),
        ({"red_noise": dict(amp=put(rn, (1, 0, 4), np.inf))}, "realization 1, pulsar 0, mode 4: non-finite amplitude"),
        ({"red_noise": dict(amp=put(rn, (1, 2, 0), 1e-7))},
         "realization 1, pulsar 2, mode 0: nonzero amplitude where the layout's is 0"),
        ({"red_noise": dict(amp=put(rn, (0, 1, 3), 1e-7))}, "realization 0, pulsar 1, mode 3: nonzero amplitude"),
        ({"gw_common": dict(log10_A=[-14, -14, np.nan, -14], gamma=3.0)}, "realization 2: non-finite log10_A"),
        ({"red_noise": dict(log10_A=-14.0, gamma=put(np.full((R, P), 3.0), (3, 1), np.inf))},
         "realization 3, pulsar 1: non-finite gamma"),
        ({"nope": dict(amp=gw)}, "spectra['nope']: unknown signal"),
        ({"gw_common": dict(amp=gw), 1: dict(amp=gw)}, "more than one table for signal 'gw_common'"),
        ({"gw_common": dict(amp=np.tile(gw[:, None, :], (1, P, 1)))}, "a per-pulsar table [R, P, N] for a common signal"),
        ({"gw_common": dict(log10_A=np.full((R, P), -14.0), gamma=3.0)}, "a per-pulsar table [R, P] for a common signal"),
        ({"gw_common": dict(amp=gw[:3])}, "3 rows for 4 realizations"),
        ({"red_noise": dict(log10_A=np.full(R + 1, -14.0), gamma=3.0)}, "5 rows for 4 realizations"),
        ({"gw_common": dict(amp=np.full((R, 5), 1e-8))}, "must end in the signal's 4 modes"),
        ({"red_noise": dict(amp=np.full((R, 2, 5), 1e-8))}, "has 2 pulsars, the layout 3"),
        ({"gw_common": dict(amp=gw, gamma=3.0)}, "expected psd, amp or (log10_A, gamma)"),
        ({"gw_common": dict(log10_A=-14.0)}, "expected psd, amp or (log10_A, gamma)"),
    ]
    for spectra, msg in cases:
        with pytest.raises(ValueError) as e:
            spectrum_tables(sim, spectra, R)
        assert msg in str(e.value), (str(e.value), msg)
    with pytest.raises(ValueError):
        spectrum_tables(sim, {"gw_common": dict(amp=gw)}, 0)
    with pytest.raises(TypeError):
        spectrum_tables(sim, [("gw_common", dict(amp=gw))], R)
    with pytest.raises(TypeError):
        spectrum_tables(sim, {"gw_common": gw}, R)


# ----------------------------------------------------------------------------- the validator, stand-alone
_MAIN = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "spectra_host.h"
// Layout: 3 pulsars; signal 0 per-pulsar, 5 modes (padded to 6), pulsar 1 carries 3 of them and pulsar 2 none; signal
// 1 common, 4 modes. Input: "n_real n_tab", then per table "seg form per_pulsar n_rows n_values v...": n_values < 0
// passes a null table. Prints "ok" or "bad reason".
int main() {
  const int P = 3;
  std::vector<double> a0((size_t)P * 6, 0.0), a1(4, 1e-8);
  for (int k = 0; k < 5; ++k) a0[k] = 1e-7;
  for (int k = 0; k < 3; ++k) a0[6 + k] = 1e-7;
  const fpta_spec::Signal sig[2] = {{0, 5, 6, a0.data()}, {1, 4, 4, a1.data()}};
  int n_real = 0, n_tab = 0;
  if (std::scanf("%d %d", &n_real, &n_tab) != 2) return 2;
  std::vector<int32_t> seg, form, per, rows;
  std::vector<std::vector<double>> store;
  std::vector<const double*> ptr;
  std::vector<char> null_tab;
  for (int t = 0; t < n_tab; ++t) {
    int s, f, pp, nr;
    long nv;
    if (std::scanf("%d %d %d %d %ld", &s, &f, &pp, &nr, &nv) != 5) return 2;
    seg.push_back(s), form.push_back(f), per.push_back(pp), rows.push_back(nr);
    null_tab.push_back(nv < 0);
    store.emplace_back((size_t)(nv < 0 ? 0 : nv));  // exactly the values given: a read past them is a sanitizer error
    for (double& v : store.back())
      if (std::scanf("%lf", &v) != 1) return 2;
  }
  for (int t = 0; t < n_tab; ++t) ptr.push_back(null_tab[t] ? nullptr : store[t].data());
  std::string why;
  const bool ok = fpta_spec::validate(P, 2, sig, n_real, n_tab, n_tab ? seg.data() : nullptr, n_tab ? form.data() : nullptr,
                                      n_tab ? per.data() : nullptr, n_tab ? rows.data() : nullptr,
                                      n_tab ? ptr.data() : nullptr, why);
  if (ok)
    std::printf("ok\n");
  else
    std::printf("bad %s\n", why.c_str());
  if (n_tab == 1 && seg[0] >= 0 && seg[0] < 2)
    std::printf("len %ld\n", (long)fpta_spec::table_len(sig[seg[0]], P, form[0], per[0], n_real));
  return 0;
}
"""


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("spectra_host")
    (d / "main.cpp").write_text(_MAIN)
    exe = str(d / "spectra_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, str(d / "main.cpp"), "-o", exe], check=True)

    def run(n_real, tables):
        text = f"{n_real} {len(tables)}\n"
        for seg, form, per, n_rows, v in tables:
            v = None if v is None else np.asarray(v, dtype=np.float64).ravel()
            text += f"{seg} {form} {per} {n_rows} {-1 if v is None else len(v)}\n"
            if v is not None:
                text += " ".join(repr(float(x)) for x in v) + "\n"
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return r.stdout.splitlines()
    return run


R = 3
_RN = np.zeros((R, 3, 5))
_RN[:, 0, :] = 2e-7
_RN[:, 1, :3] = 3e-7
_GW = np.full((R, 4), 1e-8)


def test_validator_accepts(host_program):
    assert host_program(R, []) == ["ok"]  # n_tab = 0: plain synth
    assert host_program(R, [(1, 0, 0, R, _GW)]) == ["ok", f"len {R * 4}"]
    assert host_program(R, [(0, 0, 1, R, _RN)]) == ["ok", f"len {R * 3 * 5}"]
    assert host_program(R, [(0, 0, 0, R, np.full((R, 5), 1e-7))]) == ["ok", f"len {R * 5}"]  # a shared row
    assert host_program(R, [(1, 1, 0, R, np.tile([-14.0, 0.0], (R, 1)))]) == ["ok", f"len {R * 2}"]
    assert host_program(R, [(0, 1, 1, R, np.tile([-18.0, 7.0], (R, 3, 1)))]) == ["ok", f"len {R * 3 * 2}"]
    assert host_program(R, [(0, 1, 0, R, np.tile([-14.0, 3.0], (R, 1))), (1, 0, 0, R, _GW)]) == ["ok"]
    assert host_program(R, [(1, 0, 0, R, np.zeros((R, 4)))])[0] == "ok"  # zeros are amplitudes


def test_validator_refusals(host_program):
    def one(tables, n_real=R):
        out = host_program(n_real, tables)
        assert out[0].startswith("bad "), out
        return out[0][4:]

    def put(a, idx, v):
        a = a.copy()
        a[idx] = v
        return a
    assert one([(1, 0, 0, R, put(_GW, (2, 3), np.nan))]) == "signal 1: realization 2, mode 3: non-finite amplitude"
    assert one([(1, 0, 0, R, put(_GW, (0, 0), -1e-9))]) == "signal 1: realization 0, mode 0: negative amplitude"
    assert one([(0, 0, 1, R, put(_RN, (1, 0, 4), np.inf))]) == "signal 0: realization 1, pulsar 0, mode 4: non-finite amplitude"
    assert one([(0, 0, 1, R, put(_RN, (1, 2, 0), 1e-7))]) == \
        "signal 0: realization 1, pulsar 2, mode 0: nonzero amplitude where the layout's is 0"
    assert one([(0, 0, 1, R, put(_RN, (2, 1, 3), 1e-7))]) == \
        "signal 0: realization 2, pulsar 1, mode 3: nonzero amplitude where the layout's is 0"
    assert one([(1, 1, 0, R, put(np.tile([-14.0, 3.0], (R, 1)), (1, 0), np.nan))]) == \
        "signal 1: realization 1: non-finite log10_A"
    assert one([(0, 1, 1, R, put(np.tile([-14.0, 3.0], (R, 3, 1)), (2, 1, 1), np.inf))]) == \
        "signal 0: realization 2, pulsar 1: non-finite gamma"
    assert one([(2, 0, 0, R, _GW)]).startswith("signal 2: unknown signal id")
    assert one([(-1, 0, 0, R, _GW)]).startswith("signal -1: unknown signal id")
    assert one([(1, 0, 0, R, _GW), (1, 1, 0, R, np.tile([-14.0, 3.0], (R, 1)))]) == "signal 1: more than one table"
    assert one([(1, 0, 1, R, np.tile(_GW[:, None, :], (1, 3, 1)))]) == "signal 1: a per-pulsar table for a common signal"
    assert one([(1, 0, 0, 2, _GW[:2])]) == "signal 1: 2 table rows for a block of 3 realizations"
    assert one([(1, 0, 0, 0, [])]) == "signal 1: 0 table rows for a block of 3 realizations"  # a zero-length table
    assert one([(1, 0, 0, R, None)]) == "signal 1: table missing"
    assert one([(1, 2, 0, R, _GW)]) == "signal 1: unknown table form 2"
    assert one([(0, 0, 2, R, _RN)]) == "signal 0: per_pulsar must be 0 or 1"
    assert one([(1, 0, 0, R, _GW)], n_real=0) == "bad arguments"
