// Anisotropic ORF (fpta_orf_anisotropic): ORF_m = 1.5 / npix G diag(h_m, h_m) G^T with G [P][2 npix] = [F+ | Fx] the
// antenna patterns of the pulsars over the HEALPix pixel centres, on v_mfma_f64_16x16x4_f64. G is never stored: each
// entry is ~30 flops of geometry, made in LDS chunk by chunk.
//
//   k_orf_aniso<NM>  one lower-triangle tile of 64 x 64 pulsars x one K-split of the pixel range x one group of NM maps.
//                    Per chunk of 16 pixels: 16 lanes make the pixels' geometry (ring by binary search of the ring
//                    table, cos / sin phi by sincospi of the rational multiple of pi), the workgroup generates F+ and
//                    Fx of its row-tile and column-tile pulsars (a diagonal tile: one side) into LDS, then 8 MFMA
//                    k-steps per 16 x 16 fragment and map, the map weight applied to the B operand as it is read.
//                    Accumulators stay in registers across chunks; the partial tile goes to the workspace.
//   k_orf_reduce     sums the K-split partials in ascending split order, applies 1.5 / npix and the doubled diagonal,
//                    writes both triangles from the lower one. No atomics: a repeated call is bit-identical.
// Reduction row r = 2 pixel + (0: F+, 1: Fx) of a chunk, so pixels are summed in ascending order.
#include "capi_host.h"
#include "orf_host.h"
#include "device_common.h"

namespace __attribute__((visibility("hidden"))) capi {

using fpta_orf::Ring;
constexpr int kOrfTile = fpta_orf::kTile, kOrfChunk = fpta_orf::kChunk, kOrfGroup = fpta_orf::kMapGroup;
constexpr int kOrfRows = 2 * kOrfChunk;  // reduction rows per chunk
constexpr int kOrfPitch = 80;            // LDS row pitch in doubles: 640 B = 128 mod 256, so the two 16-lane rows a
                                         // half-wave reads fall in disjoint banks
static_assert(kOrfTile == 64 && kOrfChunk == 16, "k_orf_aniso's lane maps are written for 64 x 64 tiles, 16-pixel chunks");

struct OrfArgs {
  const double* pos;   // [n_psr][3]
  const Ring* rings;   // [n_rings]
  const double* h;     // [n_map][npix]: the maps of this launch's first group onwards
  double* part;        // [group][kOrfGroup][n_split][n_tiles][64 x 64]
  int32_t n_psr, n_rings, npix, n_chunks, per_split, n_split, n_tiles;
  int32_t group0;      // workspace index of this launch's first group
};

// F+ and Fx of a pulsar for a pixel (cos phi, sin phi, z = cos theta, sin theta): the header's expression, literally
__device__ __forceinline__ void antenna(double px, double py, double pz, double cp, double sp, double z, double st,
                                        double& fplus, double& fcross) {
  const double mp = sp * px - cp * py;
  const double nq = (-z * cp) * px + (-z * sp) * py + st * pz;
  const double op = (-st * cp) * px + (-st * sp) * py - z * pz;
  const double d = 1.0 + op;
  fplus = 0.5 * (mp * mp - nq * nq) / d;
  fcross = (mp * nq) / d;
}

template <int NM>
__global__ __launch_bounds__(256) void k_orf_aniso(OrfArgs a) {
  __shared__ double sA[kOrfRows][kOrfPitch];
  __shared__ double sB[kOrfRows][kOrfPitch];
  __shared__ double sGeo[2][4][kOrfChunk];  // cos phi, sin phi, z, sin theta; two buffers by chunk parity
  __shared__ double sH[2][NM][kOrfChunk];

  const int tile = blockIdx.x, split = blockIdx.y, group = blockIdx.z;
  int bi = (int)((sqrt(8.0 * (double)tile + 1.0) - 1.0) * 0.5);
  while (bi * (bi + 1) / 2 > tile) --bi;
  while ((bi + 1) * (bi + 2) / 2 <= tile) ++bi;
  const int bj = tile - bi * (bi + 1) / 2;
  const bool diag = bi == bj;

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lg = lane >> 4;
  const int wr = wave >> 1, wc = wave & 1;
  const bool work = !(diag && wr == 0 && wc == 1);  // that quarter of a diagonal tile lies above the diagonal

  // generation: lane = pulsar of the tile, wave = pixels wave, wave + 4, ..
  const int ia = bi * kOrfTile + lane, ib = bj * kOrfTile + lane;
  double ax = 0.0, ay = 0.0, az = 0.0, bx = 0.0, by = 0.0, bz = 0.0;  // past the last pulsar: F = 0
  if (ia < a.n_psr) {
    ax = a.pos[3 * ia];
    ay = a.pos[3 * ia + 1];
    az = a.pos[3 * ia + 2];
  }
  if (ib < a.n_psr) {
    bx = a.pos[3 * ib];
    by = a.pos[3 * ib + 1];
    bz = a.pos[3 * ib + 2];
  }
  const double* __restrict__ hg = a.h + (int64_t)group * NM * a.npix;

  d4 acc[NM][2][2];
#pragma unroll
  for (int m = 0; m < NM; ++m)
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 2; ++y) acc[m][x][y] = d4{0.0, 0.0, 0.0, 0.0};

  const int c0 = split * a.per_split, c1 = min(c0 + a.per_split, a.n_chunks);
  for (int c = c0; c < c1; ++c) {
    const int buf = (c - c0) & 1;
    if (tid < kOrfChunk) {
      // a pixel past the map's end repeats the last one; its weight is 0
      const int p = min(c * kOrfChunk + tid, a.npix - 1);
      int lo = 0, hi = a.n_rings - 1;  // the last ring whose first pixel is <= p
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.rings[mid].first <= p) lo = mid; else hi = mid - 1;
      }
      const Ring r = a.rings[lo];
      FPTA_DCHECK(p - r.first < r.count, "k_orf_aniso ring", p - r.first, r.count);
      double sp, cp;
      sincospi((double)(2 * (p - r.first) + r.odd) / (double)r.count, &sp, &cp);
      sGeo[buf][0][tid] = cp;
      sGeo[buf][1][tid] = sp;
      sGeo[buf][2][tid] = r.z;
      sGeo[buf][3][tid] = r.st;
    } else if (tid >= 64 && tid < 64 + NM * kOrfChunk) {
      const int m = (tid - 64) >> 4, pl = (tid - 64) & 15;
      const int p = c * kOrfChunk + pl;
      sH[buf][m][pl] = p < a.npix ? hg[(int64_t)m * a.npix + p] : 0.0;
    }
    __syncthreads();  // the geometry is there; every wave is past the previous chunk's MFMA steps
#pragma unroll
    for (int q = 0; q < kOrfChunk / 4; ++q) {
      const int pl = wave + 4 * q;
      const double cp = sGeo[buf][0][pl], sp = sGeo[buf][1][pl], z = sGeo[buf][2][pl], st = sGeo[buf][3][pl];
      double fp, fc;
      antenna(ax, ay, az, cp, sp, z, st, fp, fc);
      sA[2 * pl][lane] = fp;
      sA[2 * pl + 1][lane] = fc;
      if (!diag) {
        antenna(bx, by, bz, cp, sp, z, st, fp, fc);
        sB[2 * pl][lane] = fp;
        sB[2 * pl + 1][lane] = fc;
      }
    }
    __syncthreads();
    if (work) {
      const double(*sBB)[kOrfPitch] = diag ? sA : sB;
#pragma unroll
      for (int kk = 0; kk < kOrfRows / 4; ++kk) {
        const int k = 4 * kk + lg;
        const double a0 = sA[k][wr * 32 + lr], a1 = sA[k][wr * 32 + 16 + lr];
        const double b0 = sBB[k][wc * 32 + lr], b1 = sBB[k][wc * 32 + 16 + lr];
#pragma unroll
        for (int m = 0; m < NM; ++m) {
          const double w = sH[buf][m][k >> 1];
          const double wb0 = b0 * w, wb1 = b1 * w;
          acc[m][0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, wb0, acc[m][0][0], 0, 0, 0);
          acc[m][0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, wb1, acc[m][0][1], 0, 0, 0);
          acc[m][1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, wb0, acc[m][1][0], 0, 0, 0);
          acc[m][1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, wb1, acc[m][1][1], 0, 0, 0);
        }
      }
    }
  }

  // the partial tile: D row = lg + 4 reg, column = lr of each fragment
#pragma unroll
  for (int m = 0; m < NM; ++m) {
    double* __restrict__ dst =
        a.part + ((((int64_t)(a.group0 + group) * kOrfGroup + m) * a.n_split + split) * a.n_tiles + tile) *
                     (kOrfTile * kOrfTile);
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 2; ++y)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          dst[(wr * 32 + x * 16 + lg + 4 * q) * kOrfTile + wc * 32 + y * 16 + lr] = acc[m][x][y][q];
  }
}

// grid (ceil(n_psr^2 / 256), maps): element (i, j <= i) of map blockIdx.y of the launch batch
__global__ __launch_bounds__(256) void k_orf_reduce(const double* __restrict__ part, int32_t n_split, int32_t n_tiles,
                                                     int32_t n_psr, double npix, double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t i = e / n_psr, j = e - i * n_psr;
  if (i >= n_psr || j > i) return;
  const int bi = (int)(i >> 6), bj = (int)(j >> 6);
  const int tile = bi * (bi + 1) / 2 + bj;
  const int mb = blockIdx.y;
  const double* __restrict__ src = part + ((int64_t)mb * n_split * n_tiles + tile) * (kOrfTile * kOrfTile) +
                                   (i & 63) * kOrfTile + (j & 63);
  double acc = 0.0;
  for (int32_t s = 0; s < n_split; ++s) acc += src[(int64_t)s * n_tiles * (kOrfTile * kOrfTile)];
  double v = 1.5 * acc / npix;
  if (i == j) v *= 2.0;
  double* __restrict__ o = out + (int64_t)mb * n_psr * n_psr;
  o[i * n_psr + j] = v;
  o[j * n_psr + i] = v;
}

template <int NM>
static hipError_t launch_orf(hipStream_t st, const OrfArgs& a, int32_t n_groups) {
  k_orf_aniso<NM><<<dim3((unsigned)a.n_tiles, (unsigned)a.n_split, (unsigned)n_groups), dim3(256), 0, st>>>(a);
  return hipGetLastError();
}

// a last group of `tail` < kOrfGroup maps
template <int NM>
static hipError_t launch_orf_tail(hipStream_t st, const OrfArgs& a, int32_t tail) {
  if (tail == NM) return launch_orf<NM>(st, a, 1);
  if constexpr (NM > 1) return launch_orf_tail<NM - 1>(st, a, tail);
  return hipErrorInvalidValue;
}

}  // namespace capi

using namespace capi;

extern "C" int fpta_healpix_pix2ang_ring(int32_t nside, int64_t n, const int64_t* ipix, double* theta_out,
                                         double* phi_out) {
  std::string why;
  if (!fpta_orf::check_nside(nside, why)) return fail(nullptr, FPTA_EINVAL, "healpix_pix2ang_ring: " + why);
  if (n < 0 || (n > 0 && (!ipix || !theta_out || !phi_out)))
    return fail(nullptr, FPTA_EINVAL, "healpix_pix2ang_ring: bad arguments");
  const int64_t npix = fpta_orf::npix_of(nside);
  for (int64_t i = 0; i < n; ++i)
    if (ipix[i] < 0 || ipix[i] >= npix)
      return fail(nullptr, FPTA_EINVAL, "healpix_pix2ang_ring: element " + std::to_string(i) + ": pixel " +
                                            std::to_string(ipix[i]) + " outside [0, " + std::to_string(npix) + ")");
  for (int64_t i = 0; i < n; ++i) fpta_orf::pix2ang(nside, ipix[i], theta_out[i], phi_out[i]);
  return FPTA_OK;
}

extern "C" int fpta_orf_plan(int32_t n_psr, int32_t nside, int64_t npix, int32_t n_map, int64_t split,
                             int64_t* info) {
  std::string why;
  if (!info) return fail(nullptr, FPTA_EINVAL, "orf_plan: bad arguments");
  if (!fpta_orf::validate_shape(n_psr, nside, npix, n_map, why)) return fail(nullptr, FPTA_EINVAL, "orf_plan: " + why);
  const fpta_orf::Plan p = fpta_orf::make_plan(n_psr, nside, n_map, split);
  const int64_t v[FPTA_ORF_PLAN_LEN] = {fpta_orf::kTile, fpta_orf::kChunk, fpta_orf::kMapGroup, p.n_tiles, p.n_chunks,
                                        p.n_split,       p.per_split,      p.n_groups,          p.launch_groups,
                                        p.part_doubles * (int64_t)sizeof(double)};
  std::copy(v, v + FPTA_ORF_PLAN_LEN, info);
  return FPTA_OK;
}

extern "C" int fpta_orf_anisotropic(fpta_ctx* c, int32_t n_psr, const double* pos, int32_t nside, int32_t n_map,
                                    const double* h_maps, double* orf_out) {
  if (!c) return fail(nullptr, FPTA_EINVAL, "null ctx");
  if (n_psr < 0 || n_map < 0 || (n_psr > 0 && !pos) || (n_map > 0 && !h_maps) || (n_psr > 0 && n_map > 0 && !orf_out))
    return fail(c, FPTA_EINVAL, "orf_anisotropic: bad arguments");
  // everything is validated here, before anything is uploaded or launched
  std::string why;
  const int64_t npix = fpta_orf::npix_of(nside);
  if (!fpta_orf::validate(n_psr, pos, nside, npix, n_map, h_maps, why))
    return fail(c, FPTA_EINVAL, "orf_anisotropic: " + why);
  if (n_psr == 0 || n_map == 0) return FPTA_OK;
  const fpta_orf::Plan plan = fpta_orf::make_plan(n_psr, nside, n_map, c->orf_split);
  const std::vector<Ring> rings = fpta_orf::ring_table(nside);
  const int64_t batch_maps = (int64_t)plan.launch_groups * kOrfGroup;
  const size_t pp = (size_t)n_psr * n_psr;

  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  int rc;
  if ((rc = upload(c, c->orf_pos, pos, sizeof(double) * 3 * n_psr, "orf pos"))) return rc;
  if ((rc = upload(c, c->orf_rings, rings.data(), sizeof(Ring) * rings.size(), "orf rings"))) return rc;
  if ((rc = upload(c, c->orf_h, h_maps, sizeof(double) * (size_t)n_map * npix, "orf maps"))) return rc;
  HIPCHK(c, c->orf_part.ensure(sizeof(double) * (size_t)plan.part_doubles), "orf partial sums");
  HIPCHK(c, c->orf_out.ensure(sizeof(double) * pp * (size_t)std::min<int64_t>(batch_maps, n_map)), "orf out");
  OrfArgs a;
  a.pos = c->orf_pos.as<double>();
  a.rings = c->orf_rings.as<Ring>();
  a.part = c->orf_part.as<double>();
  a.n_psr = n_psr;
  a.n_rings = (int32_t)rings.size();
  a.npix = (int32_t)npix;
  a.n_chunks = plan.n_chunks;
  a.per_split = plan.per_split;
  a.n_split = plan.n_split;
  a.n_tiles = plan.n_tiles;
  for (int64_t m0 = 0; m0 < n_map; m0 += batch_maps) {
    const int32_t nm = (int32_t)std::min<int64_t>(batch_maps, n_map - m0);
    const int32_t n_full = nm / kOrfGroup, tail = nm % kOrfGroup;
    {
      KTimer kt(c, FPTA_K_DENSE);
      if (n_full) {
        a.h = c->orf_h.as<double>() + m0 * npix;
        a.group0 = 0;
        HIPCHK(c, launch_orf<kOrfGroup>(c->stream, a, n_full), "k_orf_aniso launch");
      }
      if (tail) {
        a.h = c->orf_h.as<double>() + (m0 + (int64_t)n_full * kOrfGroup) * npix;
        a.group0 = n_full;
        HIPCHK(c, launch_orf_tail<(kOrfGroup > 1 ? kOrfGroup - 1 : 1)>(c->stream, a, tail), "k_orf_aniso launch");
      }
      k_orf_reduce<<<dim3((unsigned)((pp + 255) / 256), (unsigned)nm), dim3(256), 0, c->stream>>>(
          c->orf_part.as<double>(), plan.n_split, plan.n_tiles, n_psr, (double)npix, c->orf_out.as<double>());
      HIPCHK(c, hipGetLastError(), "k_orf_reduce launch");
    }
    HIPCHK(c, hipMemcpyAsync(orf_out + m0 * pp, c->orf_out.p, sizeof(double) * pp * nm, hipMemcpyDeviceToHost,
                             c->stream),
           "orf download");
  }
  HIPCHK(c, hipStreamSynchronize(c->stream), "orf sync");
  return FPTA_OK;
}
