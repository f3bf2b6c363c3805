// Per-realization spectra of a batch block (fpta_batch_synth_spectra), host side in plain C++: validation of the
// call's tables against the layout's signals. No HIP here: spectra.hip includes it, and a stand-alone CPU program can
// include it alone (tests/test_spectra_host.py builds one under the address sanitizer). Everything a call can refuse
// is refused here, before anything is uploaded or launched, so a refused call leaves the resident block as it was.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

namespace fpta_spec {

constexpr double kFyr = 1.0 / 31557600.0;  // 1 / Julian year in Hz: fakepta.constants.fyr

// One signal of the layout as the validator sees it: amp the layout's amplitudes [n_psr or 1][nmp] (nmp: n_modes
// padded to even, the padding mode's amplitude 0).
struct Signal {
  int32_t kind;     // 0 per-pulsar, 1 common
  int32_t n_modes;  // as given to add_signal
  int32_t nmp;
  const double* amp;
};

// Table t of a call: form 0 amplitudes [R][n_modes] (per_pulsar 0) or [R][n_psr][n_modes] (1); form 1
// (log10_A, gamma) [R][2] or [R][n_psr][2]
inline int64_t table_len(const Signal& s, int32_t n_psr, int32_t form, int32_t per_pulsar, int32_t n_real) {
  return (int64_t)n_real * (per_pulsar ? n_psr : 1) * (form == 0 ? s.n_modes : 2);
}

// The layout's amplitude of (pulsar p, mode k) of a signal is exactly 0: it stays 0 in every realization. For a
// table row shared by the pulsars of a per-pulsar signal (p < 0): no pulsar carries mode k.
inline bool layout_zero(const Signal& s, int32_t n_psr, int32_t p, int32_t k) {
  if (s.kind == 1) return s.amp[k] == 0.0;
  if (p >= 0) return s.amp[(int64_t)p * s.nmp + k] == 0.0;
  for (int32_t q = 0; q < n_psr; ++q)
    if (s.amp[(int64_t)q * s.nmp + k] != 0.0) return false;
  return true;
}

// Validates the tables of one call against the layout (n_psr pulsars, sig [n_sig]) and a block of n_real
// realizations. False with the reason in `why`; a bad entry is named "signal s: realization r, pulsar p, mode k:
// reason" (the pulsar only for a per-pulsar table, the mode only for an amplitude).
inline bool validate(int32_t n_psr, int32_t n_sig, const Signal* sig, int32_t n_real, int32_t n_tab,
                     const int32_t* seg, const int32_t* form, const int32_t* per_pulsar, const int32_t* n_rows,
                     const double* const* tables, std::string& why) {
  if (n_psr <= 0 || n_sig < 0 || (n_sig > 0 && !sig) || n_real <= 0 || n_tab < 0) {
    why = "bad arguments";
    return false;
  }
  if (n_tab == 0) return true;
  if (!seg || !form || !per_pulsar || !n_rows || !tables) {
    why = "bad arguments";
    return false;
  }
  std::vector<char> seen((size_t)n_sig, 0);
  for (int32_t t = 0; t < n_tab; ++t) {
    const std::string who = "signal " + std::to_string(seg[t]) + ": ";
    if (seg[t] < 0 || seg[t] >= n_sig) {
      why = who + "unknown signal id (the layout has " + std::to_string(n_sig) + ")";
      return false;
    }
    if (seen[(size_t)seg[t]]) {
      why = who + "more than one table";
      return false;
    }
    seen[(size_t)seg[t]] = 1;
    const Signal& s = sig[seg[t]];
    if (form[t] != 0 && form[t] != 1) {
      why = who + "unknown table form " + std::to_string(form[t]);
      return false;
    }
    if (per_pulsar[t] != 0 && per_pulsar[t] != 1) {
      why = who + "per_pulsar must be 0 or 1";
      return false;
    }
    if (per_pulsar[t] && s.kind == 1) {
      why = who + "a per-pulsar table for a common signal";
      return false;
    }
    if (n_rows[t] != n_real) {
      why = who + std::to_string(n_rows[t]) + " table rows for a block of " + std::to_string(n_real) + " realizations";
      return false;
    }
    if (!tables[t]) {
      why = who + "table missing";
      return false;
    }
    const int32_t np = per_pulsar[t] ? n_psr : 1;
    const double* v = tables[t];
    auto where = [&](int32_t r, int32_t p) {
      return who + "realization " + std::to_string(r) + (per_pulsar[t] ? ", pulsar " + std::to_string(p) : "");
    };
    for (int32_t r = 0; r < n_real; ++r)
      for (int32_t p = 0; p < np; ++p) {
        if (form[t] == 1) {
          const double* x = v + ((int64_t)r * np + p) * 2;
          if (!std::isfinite(x[0]) || !std::isfinite(x[1])) {
            why = where(r, p) + ": non-finite " + (std::isfinite(x[0]) ? "gamma" : "log10_A");
            return false;
          }
          continue;
        }
        const double* x = v + ((int64_t)r * np + p) * s.n_modes;
        for (int32_t k = 0; k < s.n_modes; ++k) {
          const char* bad = nullptr;
          if (!std::isfinite(x[k]))
            bad = "non-finite amplitude";
          else if (x[k] < 0.0)
            bad = "negative amplitude";
          else if (x[k] != 0.0 && layout_zero(s, n_psr, per_pulsar[t] ? p : -1, k))
            bad = "nonzero amplitude where the layout's is 0";
          if (bad) {
            why = where(r, p) + ", mode " + std::to_string(k) + ": " + bad;
            return false;
          }
        }
      }
  }
  return true;
}

}  // namespace fpta_spec
