// Anisotropic ORF (fpta_orf_anisotropic, fpta_healpix_pix2ang_ring): HEALPix RING geometry, input validation and the
// tile / K-split plan, on the host in plain C++. No HIP here: orf.hip includes it for the ring table its kernels read
// and for the plan of its launches, and a stand-alone CPU program can include it alone (tests/test_orf_host.py builds
// one under the address sanitizer). The definition is in include/fakepta_amd.h.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

namespace fpta_orf {

constexpr int32_t kNsideMax = 1024;
constexpr int32_t kPsrMax = 8192;      // pulsars of one call (the partial sums of one map group then stay below 1.1 GB)
constexpr double kUnitTol = 1e-8;      // | |p| - 1 | admitted
constexpr long double kPiL = 3.14159265358979323846264338327950288L;

inline int64_t npix_of(int64_t nside) { return 12 * nside * nside; }
inline int64_t ncap_of(int64_t nside) { return 2 * nside * (nside - 1); }

// floor(sqrt(x)) for x >= 0, exact
inline int64_t isqrt(int64_t x) {
  int64_t r = (int64_t)std::sqrt((double)x);
  while (r * r > x) --r;
  while ((r + 1) * (r + 1) <= x) ++r;
  return r;
}

// Ring i = 1 .. 4 nside - 1 and the 1-based index j in it of pixel p (0 <= p < npix), the header's three cases.
struct RingPos {
  int64_t ring, j;
};
inline RingPos pix_ring(int64_t nside, int64_t p) {
  const int64_t npix = npix_of(nside), ncap = ncap_of(nside);
  if (p < ncap) {
    const int64_t i = (1 + isqrt(1 + 2 * p)) >> 1;
    return {i, p + 1 - 2 * i * (i - 1)};
  }
  if (p < npix - ncap) {
    const int64_t q = p - ncap, t = q / (4 * nside);
    return {t + nside, q - 4 * nside * t + 1};
  }
  const int64_t q = npix - p, i = (1 + isqrt(2 * q - 1)) >> 1;
  return {4 * nside - i, 4 * i + 1 - (q - 2 * i * (i - 1))};
}

// One ring as the kernels read it: z = cos(theta) and sin(theta) rounded once from long double, the first pixel, the
// pixel count, and phi of the ring's pixel with 0-based index j0 as the rational (2 j0 + odd) / count times pi
// (caps: (j - 1/2) pi / (2 i) with count = 4 i; belt: (j - s) pi / (2 nside) with count = 4 nside, odd = 2 - 2 s).
struct Ring {
  double z, st;
  int32_t first, count, odd, pad;
};
static_assert(sizeof(Ring) == 32, "Ring is the device table row");

// z and sin(theta) of ring i in long double
inline void ring_z(int64_t nside, int64_t i, long double& z, long double& st) {
  const long double npix = (long double)npix_of(nside);
  if (i < nside) {
    z = 1.0L - (long double)(4 * i * i) / npix;
  } else if (i <= 3 * nside) {
    z = (long double)(2 * nside - i) * 2.0L / (long double)(3 * nside);
  } else {
    const int64_t k = 4 * nside - i;
    z = -1.0L + (long double)(4 * k * k) / npix;
  }
  st = std::sqrt((1.0L - z) * (1.0L + z));
}

inline Ring ring_row(int64_t nside, int64_t i) {
  long double z, st;
  ring_z(nside, i, z, st);
  Ring r;
  r.z = (double)z;
  r.st = (double)st;
  r.pad = 0;
  if (i < nside) {
    r.first = (int32_t)(2 * i * (i - 1));
    r.count = (int32_t)(4 * i);
    r.odd = 1;
  } else if (i <= 3 * nside) {
    r.first = (int32_t)(ncap_of(nside) + (i - nside) * 4 * nside);
    r.count = (int32_t)(4 * nside);
    r.odd = (int32_t)(((i + nside) & 1) ? 0 : 1);  // s = 1 when i + nside is odd, else 1/2
  } else {
    const int64_t k = 4 * nside - i;
    r.first = (int32_t)(npix_of(nside) - 2 * k * (k + 1));
    r.count = (int32_t)(4 * k);
    r.odd = 1;
  }
  return r;
}

// The per-ring table: 4 nside - 1 rows, ring i at row i - 1
inline std::vector<Ring> ring_table(int32_t nside) {
  std::vector<Ring> t((size_t)(4 * nside - 1));
  for (int64_t i = 1; i <= 4 * (int64_t)nside - 1; ++i) t[(size_t)(i - 1)] = ring_row(nside, i);
  return t;
}

// The pixel of (ring i, 1-based j): the inverse of pix_ring
inline int64_t ring_pix(int64_t nside, int64_t i, int64_t j) { return ring_row(nside, i).first + j - 1; }

// theta = atan2(sin theta, z) and phi of pixel p, each rounded once from long double
inline void pix2ang(int64_t nside, int64_t p, double& theta, double& phi) {
  const RingPos rp = pix_ring(nside, p);
  const Ring r = ring_row(nside, rp.ring);
  long double z, st;
  ring_z(nside, rp.ring, z, st);
  theta = (double)std::atan2(st, z);
  phi = (double)((long double)(2 * (rp.j - 1) + r.odd) * kPiL / (long double)r.count);
}

// ----------------------------------------------------------------------------- validation
inline bool check_nside(int64_t nside, std::string& why) {
  if (nside < 1 || nside > kNsideMax) {
    why = "nside " + std::to_string(nside) + " outside [1, " + std::to_string(kNsideMax) + "]";
    return false;
  }
  return true;
}

// nside of a map of npix pixels, or 0 when npix is not 12 nside^2 for an nside >= 1
inline int64_t npix2nside(int64_t npix) {
  if (npix < 12 || npix % 12) return 0;
  const int64_t n = isqrt(npix / 12);
  return n * n * 12 == npix ? n : 0;
}

// The shape of a call: nside, the map length, the counts. False with the reason in why.
inline bool validate_shape(int64_t n_psr, int64_t nside, int64_t npix, int64_t n_map, std::string& why) {
  if (!check_nside(nside, why)) return false;
  if (npix != npix_of(nside)) {
    why = "npix " + std::to_string(npix) + " is not 12 nside^2 = " + std::to_string(npix_of(nside));
    return false;
  }
  if (n_psr < 0 || n_psr > kPsrMax) {
    why = "n_psr " + std::to_string(n_psr) + " outside [0, " + std::to_string(kPsrMax) + "]";
    return false;
  }
  if (n_map < 0) {
    why = "n_map < 0";
    return false;
  }
  return true;
}

// Everything fpta_orf_anisotropic refuses, in the order it is checked: the shape, the positions, the maps.
inline bool validate(int64_t n_psr, const double* pos, int64_t nside, int64_t npix, int64_t n_map, const double* h_maps,
                     std::string& why) {
  if (!validate_shape(n_psr, nside, npix, n_map, why)) return false;
  for (int64_t p = 0; p < n_psr; ++p) {
    const double x = pos[3 * p], y = pos[3 * p + 1], z = pos[3 * p + 2];
    if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(z)) {
      why = "pulsar " + std::to_string(p) + ": position not finite";
      return false;
    }
    if (!(std::fabs(std::sqrt(x * x + y * y + z * z) - 1.0) <= kUnitTol)) {
      why = "pulsar " + std::to_string(p) + ": position is not a unit vector";
      return false;
    }
  }
  for (int64_t m = 0; m < n_map; ++m)
    for (int64_t i = 0; i < npix; ++i)
      if (!std::isfinite(h_maps[m * npix + i])) {
        why = "map " + std::to_string(m) + ", pixel " + std::to_string(i) + ": not finite";
        return false;
      }
  return true;
}

// ----------------------------------------------------------------------------- the plan
// Output tiles of kTile x kTile pulsars over the lower triangle (tile t = bi (bi + 1) / 2 + bj, bj <= bi); the pixel
// range in chunks of kChunk pixels (2 kChunk reduction rows: F+ and Fx of each), split into n_split contiguous runs of
// chunks; maps in groups of kMapGroup (accumulators of one group stay in registers). A pure function of its arguments;
// the split count does not depend on n_map, so a map's sums are the same whichever maps share its call.
// Variant builds may change the three tuning figures (make variant DEFS=-DFPTA_ORF_MAP_GROUP=2, ...): DESIGN.md §9.
#ifndef FPTA_ORF_MAP_GROUP
#define FPTA_ORF_MAP_GROUP 4  // 1 .. 4
#endif
#ifndef FPTA_ORF_TARGET_BLOCKS
#define FPTA_ORF_TARGET_BLOCKS 768
#endif
#ifndef FPTA_ORF_MIN_CHUNKS
#define FPTA_ORF_MIN_CHUNKS 8
#endif
constexpr int32_t kTile = 64, kChunk = 16, kMapGroup = FPTA_ORF_MAP_GROUP;
static_assert(kMapGroup >= 1 && kMapGroup <= 4, "the accumulators of one map group stay in registers");
constexpr int64_t kTargetBlocks = FPTA_ORF_TARGET_BLOCKS;    // auto: splits until about this many workgroups per map group
constexpr int64_t kMinChunksPerSplit = FPTA_ORF_MIN_CHUNKS;  // auto: each split keeps at least this many chunks
constexpr int64_t kLaunchBytes = (int64_t)256 << 20;  // partial sums of one launch (several map groups) stay below this

struct Plan {
  int32_t n_tr = 0;        // tile rows
  int32_t n_tiles = 0;     // lower-triangle tiles
  int32_t n_chunks = 0;    // pixel chunks
  int32_t per_split = 0;   // chunks per split (the last split may hold fewer)
  int32_t n_split = 0;     // splits in use (no empty trailing split)
  int32_t n_groups = 0;    // map groups
  int32_t launch_groups = 0;  // map groups per launch
  int64_t part_doubles = 0;   // partial sums of one launch: [launch_groups kMapGroup][n_split][n_tiles][kTile kTile]
};

inline Plan make_plan(int64_t n_psr, int64_t nside, int64_t n_map, int64_t option) {
  Plan p;
  if (n_psr <= 0 || nside < 1 || n_map <= 0) return p;
  p.n_tr = (int32_t)((n_psr + kTile - 1) / kTile);
  p.n_tiles = (int32_t)((int64_t)p.n_tr * (p.n_tr + 1) / 2);
  p.n_chunks = (int32_t)((npix_of(nside) + kChunk - 1) / kChunk);
  int64_t n = 1;
  if (option >= 1) {
    n = option;
  } else {
    n = (kTargetBlocks + p.n_tiles - 1) / p.n_tiles;
    const int64_t cap = p.n_chunks / kMinChunksPerSplit;
    if (n > cap) n = cap;
  }
  if (n > p.n_chunks) n = p.n_chunks;
  if (n > 65535) n = 65535;
  if (n < 1) n = 1;
  p.per_split = (int32_t)((p.n_chunks + n - 1) / n);
  p.n_split = (p.n_chunks + p.per_split - 1) / p.per_split;
  p.n_groups = (int32_t)((n_map + kMapGroup - 1) / kMapGroup);
  const int64_t group_doubles = (int64_t)kMapGroup * p.n_split * p.n_tiles * kTile * kTile;
  int64_t lg = kLaunchBytes / (group_doubles * (int64_t)sizeof(double));
  if (lg < 1) lg = 1;
  if (lg > p.n_groups) lg = p.n_groups;
  if (lg > 65535) lg = 65535;
  p.launch_groups = (int32_t)lg;
  p.part_doubles = group_doubles * lg;
  return p;
}

// (bi, bj) of lower-triangle tile t
inline void tile_of(int32_t t, int32_t& bi, int32_t& bj) {
  int32_t q = (int32_t)((std::sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while ((int64_t)q * (q + 1) / 2 > t) --q;
  while ((int64_t)(q + 1) * (q + 2) / 2 <= t) ++q;
  bi = q;
  bj = t - (int32_t)((int64_t)q * (q + 1) / 2);
}

// chunks [c0, c1) of split s
inline void split_range(const Plan& p, int32_t s, int32_t& c0, int32_t& c1) {
  c0 = s * p.per_split;
  c1 = c0 + p.per_split < p.n_chunks ? c0 + p.per_split : p.n_chunks;
}

}  // namespace fpta_orf
