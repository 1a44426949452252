// geometry.hip -- the geometry evaluation of the reference (evaluate_gs_geometry.py with dsmr.py) on the device, three stages:
//   1. depth map -> height grid (DSM) with NO point cloud in between: depth_to_point_cloud (:132-215) and
//      create_dsm_manual_satnerf_style (:270-312) fused, one thread per pixel, float64 in the reference's order;
//      mode MAX: 64-bit atomic max on an order-preserving integer key of the height (exact, order independent);
//      mode MEAN: int64 fixed point (2^-20 m) + uint32 count with integer atomics (deterministic from run to run);
//   2. dsmr.compute_shift: 2x pyramid (downsample2x), per level all (2 irange + 1)^2 shifts of mean_std in one launch per
//      pass -- a workgroup stages a 32 x 32 tile of u and the matching tile of v with its halo in LDS, every lane owns one
//      shift and keeps its float64 sums in registers -- per-tile partials added by one workgroup in tile order. No float
//      atomics: the shift cannot depend on scheduling. A level reads the level below's (dx, dy) from device memory.
//   3. apply_shift_ and compute_dsm_metrics / register_dsms_simple: a masked reduction with per-workgroup partials added in
//      a fixed order; with a shift the shifted prediction is formed on the fly.
// Every index is range-checked before it is used: a grid cell before its atomic, a raster pixel before its load (valnan).
// The kernels have no profiler ids (the id list of sfgs_profile_kernel_name is closed by the loss kernels).
#include "sfgs_internal.h"
#include "geo_unproject.h"

#include <math.h>

namespace sfgs {

constexpr int GEO_THREADS = 256;
constexpr int GEO_TILE = 32;             // u pixels per tile edge of the correlation kernels
constexpr int GEO_MAX_IRANGE = 7;        // (2 * 7 + 1)^2 = 225 shifts <= GEO_THREADS
constexpr int GEO_VT = GEO_TILE + 2 * GEO_MAX_IRANGE;
constexpr int GEO_MAX_LEVELS = 16;
constexpr int GEO_METRIC_MAX_BLOCKS = 1024;
constexpr double GEO_FIX = 1048576.0;    // fixed-point units per metre (2^20)

__device__ __forceinline__ double geo_nan() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ __forceinline__ bool geo_finite(double x) { return fabs(x) < INFINITY; }   // false for NaN and +-inf

// ---- stage 1: depth -> DSM accumulators ----------------------------------------------------------------------------------------
struct DsmView {
  GeoCamera cam;
  double xoff, yoff_top, res;
  int H, W, xsize, ysize, radius;
};

// order-preserving key of a float64: a < b <=> key(a) < key(b); no number has key 0 (= an empty cell)
__device__ __forceinline__ unsigned long long dsm_key(double h) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(h);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double dsm_unkey(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)b);
}

template <bool MEAN>
__global__ void __launch_bounds__(GEO_THREADS)
dsm_accumulate_kernel(const float* __restrict__ depth, const unsigned char* __restrict__ mask, DsmView v,
                      unsigned long long* __restrict__ acc, uint32_t* __restrict__ cnt,
                      unsigned long long* __restrict__ num_points) {
  const long long P = (long long)v.H * v.W;
  const long long p = (long long)blockIdx.x * GEO_THREADS + threadIdx.x;
  bool landed = false;
  if (p < P) {
    float d;
    if (geo_pixel_used(depth, mask, p, &d)) {
      const int row = (int)(p / v.W), col = (int)(p - (long long)row * v.W);
      double w[3];
      geo_unproject(v.cam, row, col, d, w);   // geo_unproject.h: shared with pointcloud.hip
      int gx, gy;
      if (geo_cell(w[0], w[1], v.xoff, v.yoff_top, v.res, v.xsize, v.ysize, &gx, &gy)) {   // geo_unproject.h: shared with ortho.hip
        landed = true;
        if (!MEAN) {
          atomicMax(&acc[(size_t)gy * v.xsize + gx], dsm_key(w[2]));
        } else {
          const unsigned long long q = (unsigned long long)llrint(w[2] * GEO_FIX);   // two's complement: the sum wraps like int64
          for (int dy = -v.radius; dy <= v.radius; ++dy) {
            const int cy = gy + dy;
            if (cy < 0 || cy >= v.ysize) continue;
            for (int dx = -v.radius; dx <= v.radius; ++dx) {
              const int cx = gx + dx;
              if (cx < 0 || cx >= v.xsize) continue;
              const size_t cell = (size_t)cy * v.xsize + cx;
              atomicAdd(&acc[cell], q);
              atomicAdd(&cnt[cell], 1u);
            }
          }
        }
      }
    }
  }
  const unsigned long long b = __ballot(landed);
  if (lane_id() == 0 && b) atomicAdd(num_points, (unsigned long long)__popcll(b));
}

template <bool MEAN>
__global__ void __launch_bounds__(GEO_THREADS)
dsm_finalize_kernel(const unsigned long long* __restrict__ acc, const uint32_t* __restrict__ cnt, long long cells,
                    double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * GEO_THREADS + threadIdx.x;
  if (i >= cells) return;
  double r = geo_nan();
  if (!MEAN) {
    const unsigned long long k = acc[i];
    if (k) r = dsm_unkey(k);
  } else {
    const uint32_t n = cnt[i];
    if (n) r = (double)(long long)acc[i] * (1.0 / GEO_FIX) / (double)n;
  }
  out[i] = r;
}

// ---- stage 2: registration -----------------------------------------------------------------------------------------------------
// dsmr.valnan: the pixel (row j, column i) or NaN
__device__ __forceinline__ double geo_valnan(const double* __restrict__ u, int H, int W, long long i, long long j) {
  return (i >= 0 && j >= 0 && i < W && j < H) ? u[j * W + i] : geo_nan();
}

// dsmr.downsample2x: the reference's loop writes out[j // 2, i // 2] for EVERY (j, i), so the last write wins: cell (J, I)
// is the finite-mean of the 2 x 2 window whose corner is the last pixel of {2J, 2J+1} x {2I, 2I+1} inside the raster.
__global__ void __launch_bounds__(GEO_THREADS)
dsmr_downsample_kernel(const double* __restrict__ u, int H, int W, double* __restrict__ out, int Ho, int Wo) {
  const long long idx = (long long)blockIdx.x * GEO_THREADS + threadIdx.x;
  if (idx >= (long long)Ho * Wo) return;
  const int J = (int)(idx / Wo), I = (int)(idx - (long long)J * Wo);
  const int j0 = 2 * J + 1 < H ? 2 * J + 1 : H - 1, i0 = 2 * I + 1 < W ? 2 * I + 1 : W - 1;
  double s = 0.0;
  int n = 0;
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int l = 0; l < 2; ++l) {
      const double t = geo_valnan(u, H, W, i0 + k, j0 + l);
      if (geo_finite(t)) { s = s + t; ++n; }
    }
  out[idx] = n > 0 ? s / (double)n : geo_nan();
}

struct DsmrLevel {
  const double* u; const double* v;
  int Hu, Wu, Hv, Wv;
  int irange;
  int init_dx, init_dy;        // used when `below` is NULL
  const int* below;            // (dx, dy) of the level below on the device: this level starts at twice that
  int tiles_x, tiles;
};

__device__ __forceinline__ void dsmr_init(const DsmrLevel& L, int& dx, int& dy) {
  if (L.below) { dx = L.below[0] * 2; dy = L.below[1] * 2; }
  else { dx = L.init_dx; dy = L.init_dy; }
}

// stage the workgroup's tile of u and of v (origin shifted by init - irange, edge TILE + 2 irange); pixels outside a raster: NaN
__device__ __forceinline__ void dsmr_stage(const DsmrLevel& L, double* su, double* sv, int dx0, int dy0) {
  const int tx = blockIdx.x % L.tiles_x, ty = blockIdx.x / L.tiles_x;
  const int i0 = tx * GEO_TILE, j0 = ty * GEO_TILE;
  for (int t = threadIdx.x; t < GEO_TILE * GEO_TILE; t += GEO_THREADS) {
    const int lj = t / GEO_TILE, li = t % GEO_TILE;
    su[t] = geo_valnan(L.u, L.Hu, L.Wu, i0 + li, j0 + lj);
  }
  const int VW = GEO_TILE + 2 * L.irange;
  const long long vi0 = (long long)i0 + dx0 - L.irange, vj0 = (long long)j0 + dy0 - L.irange;
  for (int t = threadIdx.x; t < VW * VW; t += GEO_THREADS) {
    const int lj = t / VW, li = t % VW;
    sv[t] = geo_valnan(L.v, L.Hv, L.Wv, vi0 + li, vj0 + lj);
  }
  __syncthreads();
}

// PASS 1: per (tile, shift) sum of u, sum of v, pair count over the pairs with both values finite.
// PASS 2: the centred sums (u - mu_u)^2, (v - mu_v)^2, (u - mu_u)(v - mu_v) with the means of pass 1.
// part: [3][tiles][nshift]; mean: [3][nshift] = (mu_u, mu_v, count)
template <int PASS>
__global__ void __launch_bounds__(GEO_THREADS)
dsmr_tile_kernel(DsmrLevel L, const double* __restrict__ mean, double* __restrict__ part) {
  __shared__ double su[GEO_TILE * GEO_TILE];
  __shared__ double sv[GEO_VT * GEO_VT];
  int dx0, dy0;
  dsmr_init(L, dx0, dy0);
  dsmr_stage(L, su, sv, dx0, dy0);
  const int S = 2 * L.irange + 1, nshift = S * S, VW = GEO_TILE + 2 * L.irange;
  const int s = threadIdx.x;
  if (s >= nshift) return;
  const int sy = s / S, sx = s % S;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, mu = 0.0, mv = 0.0;
  bool live = true;
  if (PASS == 2) { mu = mean[s]; mv = mean[nshift + s]; live = mean[2 * nshift + s] > 0.0; }
  if (live) {
    for (int lj = 0; lj < GEO_TILE; ++lj) {
      const double* vrow = sv + (lj + sy) * VW + sx;
      for (int li = 0; li < GEO_TILE; ++li) {
        const double uu = su[lj * GEO_TILE + li];     // the same address in every lane: a broadcast
        if (!geo_finite(uu)) continue;                // wave-uniform
        const double vv = vrow[li];                   // consecutive lanes (sx): consecutive addresses
        if (!geo_finite(vv)) continue;
        if (PASS == 1) { a0 = a0 + uu; a1 = a1 + vv; a2 = a2 + 1.0; }
        else {
          const double du = uu - mu, dv = vv - mv;
          a0 = a0 + du * du; a1 = a1 + dv * dv; a2 = a2 + du * dv;
        }
      }
    }
  }
  const size_t plane = (size_t)L.tiles * nshift, at = (size_t)blockIdx.x * nshift + s;
  part[at] = a0; part[plane + at] = a1; part[2 * plane + at] = a2;
}

// one workgroup; thread s adds the partials of shift s in tile order
__device__ __forceinline__ void dsmr_sum_tiles(const double* __restrict__ part, int tiles, int nshift, int s, double (&a)[3]) {
  const size_t plane = (size_t)tiles * nshift;
  a[0] = a[1] = a[2] = 0.0;
  for (int t = 0; t < tiles; ++t) {
    const size_t at = (size_t)t * nshift + s;
    a[0] = a[0] + part[at]; a[1] = a[1] + part[plane + at]; a[2] = a[2] + part[2 * plane + at];
  }
}

__global__ void __launch_bounds__(GEO_THREADS)
dsmr_mean_kernel(const double* __restrict__ part, int tiles, int nshift, double* __restrict__ mean) {
  const int s = threadIdx.x;
  if (s >= nshift) return;
  double a[3];
  dsmr_sum_tiles(part, tiles, nshift, s, a);
  const bool any = a[2] > 0.0;
  mean[s] = any ? a[0] / a[2] : geo_nan();
  mean[nshift + s] = any ? a[1] / a[2] : geo_nan();
  mean[2 * nshift + s] = a[2];
}

// sigma, xcorr and the score of every shift, then dsmr.compute_ncc's scan: y outer, x inner, strict >, so the first maximum
// wins and a NaN never does; a shift with no finite pair or sigma_u sigma_v == 0 (where the reference divides by zero) is skipped.
// shift_out[2] = the level's (dx, dy) (its start when every shift was skipped); stats_out[8] = a, b, mu_u, mu_v, sigma_u,
// sigma_v, xcorr, score at that shift (NaN when every shift was skipped; a = 1 without scaling).
__global__ void __launch_bounds__(GEO_THREADS)
dsmr_select_kernel(DsmrLevel L, const double* __restrict__ part, const double* __restrict__ mean, int scaling,
                   int* __restrict__ shift_out, double* __restrict__ stats_out) {
  __shared__ double score[GEO_THREADS], sgu[GEO_THREADS], sgv[GEO_THREADS], xc[GEO_THREADS];
  __shared__ int ok[GEO_THREADS];
  const int S = 2 * L.irange + 1, nshift = S * S;
  const int s = threadIdx.x;
  if (s < nshift) {
    double a[3];
    dsmr_sum_tiles(part, L.tiles, nshift, s, a);
    const double n = mean[2 * nshift + s];
    int good = 0;
    double su_ = geo_nan(), sv_ = geo_nan(), x_ = geo_nan(), sc = geo_nan();
    if (n > 0.0) {
      su_ = sqrt(a[0] / n); sv_ = sqrt(a[1] / n); x_ = a[2] / n;
      const double den = su_ * sv_;
      if (den != 0.0) { sc = x_ / den; good = 1; }
    }
    score[s] = sc; sgu[s] = su_; sgv[s] = sv_; xc[s] = x_; ok[s] = good;
  }
  __syncthreads();
  if (s != 0) return;
  int dx0, dy0;
  dsmr_init(L, dx0, dy0);
  int best = -1;
  double maxv = -INFINITY;
  for (int t = 0; t < nshift; ++t)
    if (ok[t] && score[t] > maxv) { best = t; maxv = score[t]; }
  const double nan = geo_nan();
  if (best < 0) {
    shift_out[0] = dx0; shift_out[1] = dy0;
    stats_out[0] = scaling ? nan : 1.0;
    for (int k = 1; k < 8; ++k) stats_out[k] = nan;
    return;
  }
  shift_out[0] = dx0 - L.irange + best % S;
  shift_out[1] = dy0 - L.irange + best / S;
  const double mu = mean[best], mv = mean[nshift + best];
  const double a = scaling ? sgu[best] / sgv[best] : 1.0;
  stats_out[0] = a;
  stats_out[1] = mu - mv * a;
  stats_out[2] = mu; stats_out[3] = mv; stats_out[4] = sgu[best]; stats_out[5] = sgv[best]; stats_out[6] = xc[best];
  stats_out[7] = score[best];
}

// ---- stage 3: shift + compare --------------------------------------------------------------------------------------------------
// dsmr.apply_shift_ with c = d = 0: a * valnan(v, i + dx, j + dy) + b (+ 0: the reference's two zero terms turn -0 into +0)
__device__ __forceinline__ double geo_shifted(const double* __restrict__ v, int H, int W, int i, int j, int dx, int dy, double a,
                                              double b) {
  const double t = a * geo_valnan(v, H, W, (long long)i + dx, (long long)j + dy);
  return (t + b) + 0.0;
}

__global__ void __launch_bounds__(GEO_THREADS)
dsm_apply_shift_kernel(const double* __restrict__ v, int H, int W, const int* __restrict__ shift, const double* __restrict__ ab,
                       double* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * GEO_THREADS + threadIdx.x;
  if (idx >= (long long)H * W) return;
  const int j = (int)(idx / W), i = (int)(idx - (long long)j * W);
  out[idx] = geo_shifted(v, H, W, i, j, shift[0], shift[1], ab[0], ab[1]);
}

// partial: [5][blocks] = sum |p - g|, sum (p - g)^2, sum (g - p), pixels valid in both, pixels valid in gt
__global__ void __launch_bounds__(GEO_THREADS)
dsm_metrics_kernel(const double* __restrict__ pred, const double* __restrict__ gt, const unsigned char* __restrict__ mask, int H,
                   int W, const int* __restrict__ shift, const double* __restrict__ ab, double* __restrict__ partial) {
  __shared__ double red[5][GEO_THREADS];
  const long long P = (long long)H * W, stride = (long long)gridDim.x * GEO_THREADS;
  int dx = 0, dy = 0;
  double a = 1.0, b = 0.0;
  if (shift) { dx = shift[0]; dy = shift[1]; a = ab[0]; b = ab[1]; }
  double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (long long idx = (long long)blockIdx.x * GEO_THREADS + threadIdx.x; idx < P; idx += stride) {
    if (mask && mask[idx] == 0) continue;
    const double g = gt[idx];
    if (g != g) continue;
    acc[4] = acc[4] + 1.0;
    double p;
    if (shift) {
      const int j = (int)(idx / W), i = (int)(idx - (long long)j * W);
      p = geo_shifted(pred, H, W, i, j, dx, dy, a, b);
    } else {
      p = pred[idx];
    }
    if (p != p) continue;
    const double d = p - g;
    acc[0] = acc[0] + fabs(d); acc[1] = acc[1] + d * d; acc[2] = acc[2] + (g - p); acc[3] = acc[3] + 1.0;
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) red[k][threadIdx.x] = acc[k];
  __syncthreads();
  for (int w = GEO_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
#pragma unroll
      for (int k = 0; k < 5; ++k) red[k][threadIdx.x] = red[k][threadIdx.x] + red[k][threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x < 5) partial[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = red[threadIdx.x][0];
}

// out[5] = mae, rmse, valid_pixels, completeness, dz (mean of gt - pred: register_dsms_simple)
__global__ void __launch_bounds__(64)
dsm_metrics_final_kernel(const double* __restrict__ partial, int blocks, double* __restrict__ out) {
  __shared__ double tot[5];
  if (threadIdx.x < 5) {
    double s = 0.0;
    for (int b = 0; b < blocks; ++b) s = s + partial[(size_t)threadIdx.x * blocks + b];
    tot[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double n = tot[3], ngt = tot[4];
  const bool any = n > 0.0;
  out[0] = any ? tot[0] / n : geo_nan();
  out[1] = any ? sqrt(tot[1] / n) : geo_nan();
  out[2] = n;
  out[3] = (any && ngt > 0.0) ? n / ngt : 0.0;
  out[4] = any ? tot[2] / n : 0.0;
}

}  // namespace sfgs

using namespace sfgs;

namespace {

inline unsigned geo_blocks(long long n) { return (unsigned)((n + GEO_THREADS - 1) / GEO_THREADS); }

int dsm_check_grid(int32_t xsize, int32_t ysize) {
  SFGS_REQUIRE(xsize > 0 && ysize > 0, SFGS_E_ARG, "DSM grid: xsize %d, ysize %d", xsize, ysize);
  SFGS_REQUIRE((long long)xsize * ysize <= (1ll << 28), SFGS_E_UNSUPPORTED, "DSM grid: xsize * ysize must not exceed 2^28, got %d x %d",
               xsize, ysize);
  return SFGS_OK;
}

int geo_check_raster(const char* what, int32_t H, int32_t W) {
  SFGS_REQUIRE(H > 0 && W > 0, SFGS_E_ARG, "%s: H %d, W %d", what, H, W);
  SFGS_REQUIRE(H <= 32768 && W <= 32768, SFGS_E_UNSUPPORTED, "%s: H and W must not exceed 32768, got %d x %d", what, H, W);
  return SFGS_OK;
}

struct DsmrPlan {
  int levels;                                   // pyramid levels including the input
  int Hu[GEO_MAX_LEVELS], Wu[GEO_MAX_LEVELS], Hv[GEO_MAX_LEVELS], Wv[GEO_MAX_LEVELS];
  size_t off_u[GEO_MAX_LEVELS], off_v[GEO_MAX_LEVELS];   // levels >= 1 live in the scratch
  size_t off_part, off_mean, off_shift, off_stats, total;
  int nshift;
};

int dsmr_plan(const SfgsDsmrArgs* a, DsmrPlan* p) {
  SFGS_REQUIRE(a, SFGS_E_ARG, "NULL SfgsDsmrArgs");
  SFGS_REQUIRE(a->struct_size == sizeof(SfgsDsmrArgs), SFGS_E_ARG, "SfgsDsmrArgs.struct_size %u, expected %zu", a->struct_size,
               sizeof(SfgsDsmrArgs));
  if (const int rc = geo_check_raster("SfgsDsmrArgs ref", a->ref_h, a->ref_w)) return rc;
  if (const int rc = geo_check_raster("SfgsDsmrArgs sec", a->sec_h, a->sec_w)) return rc;
  SFGS_REQUIRE(a->irange >= 1 && a->irange <= GEO_MAX_IRANGE, SFGS_E_ARG, "SfgsDsmrArgs.irange %d: 1 ... %d", a->irange,
               GEO_MAX_IRANGE);
  SFGS_REQUIRE(a->init_dx >= -(1 << 20) && a->init_dx <= (1 << 20) && a->init_dy >= -(1 << 20) && a->init_dy <= (1 << 20),
               SFGS_E_ARG, "SfgsDsmrArgs: init (%d, %d) beyond +-2^20", a->init_dx, a->init_dy);
  SFGS_REQUIRE(a->ref && a->sec, SFGS_E_ARG, "SfgsDsmrArgs: ref or sec is NULL");
  p->nshift = (2 * a->irange + 1) * (2 * a->irange + 1);
  p->levels = 1;
  p->Hu[0] = a->ref_h; p->Wu[0] = a->ref_w; p->Hv[0] = a->sec_h; p->Wv[0] = a->sec_w;
  size_t off = 0;
  p->off_u[0] = p->off_v[0] = 0;
  while ((p->Hu[p->levels - 1] < p->Wu[p->levels - 1] ? p->Hu[p->levels - 1] : p->Wu[p->levels - 1]) > 100) {
    const int k = p->levels;   // cannot reach GEO_MAX_LEVELS: 32768 / 2^9 < 100
    p->Hu[k] = (p->Hu[k - 1] + 1) / 2; p->Wu[k] = (p->Wu[k - 1] + 1) / 2;
    p->Hv[k] = (p->Hv[k - 1] + 1) / 2; p->Wv[k] = (p->Wv[k - 1] + 1) / 2;
    p->off_u[k] = off; off += align_up((size_t)p->Hu[k] * p->Wu[k] * 8, 256);
    p->off_v[k] = off; off += align_up((size_t)p->Hv[k] * p->Wv[k] * 8, 256);
    ++p->levels;
  }
  const size_t tiles0 = (size_t)((a->ref_h + GEO_TILE - 1) / GEO_TILE) * ((a->ref_w + GEO_TILE - 1) / GEO_TILE);
  p->off_part = off; off += align_up(3 * tiles0 * p->nshift * 8, 256);
  p->off_mean = off; off += align_up((size_t)3 * p->nshift * 8, 256);
  p->off_shift = off; off += align_up((size_t)GEO_MAX_LEVELS * 2 * 4, 256);
  p->off_stats = off; off += align_up((size_t)GEO_MAX_LEVELS * 8 * 8, 256);
  p->total = off;
  return SFGS_OK;
}

inline int floordiv2(int x) { return x >> 1; }   // Python's x // 2 (arithmetic shift: floor, also for negatives)

}  // namespace

extern "C" int sfgs_dsm_accumulate(const SfgsDsmViewArgs* a, void* acc, uint32_t* count, unsigned long long* num_points,
                                   void* stream_) {
  SFGS_REQUIRE(a, SFGS_E_ARG, "NULL SfgsDsmViewArgs");
  SFGS_REQUIRE(a->struct_size == sizeof(SfgsDsmViewArgs), SFGS_E_ARG, "SfgsDsmViewArgs.struct_size %u, expected %zu",
               a->struct_size, sizeof(SfgsDsmViewArgs));
  SFGS_REQUIRE(a->H > 0 && a->W > 0, SFGS_E_ARG, "SfgsDsmViewArgs: H %d, W %d", a->H, a->W);
  SFGS_REQUIRE((long long)a->H * a->W <= (1ll << 30), SFGS_E_UNSUPPORTED, "SfgsDsmViewArgs: H * W must not exceed 2^30, got %d x %d",
               a->H, a->W);
  if (const int rc = dsm_check_grid(a->xsize, a->ysize)) return rc;
  SFGS_REQUIRE(a->mode == SFGS_DSM_MAX || a->mode == SFGS_DSM_MEAN, SFGS_E_ARG, "SfgsDsmViewArgs.mode %d", a->mode);
  SFGS_REQUIRE(a->radius >= 0 && a->radius <= 3, SFGS_E_ARG, "SfgsDsmViewArgs.radius %d: 0 ... 3", a->radius);
  SFGS_REQUIRE(a->resolution > 0.0 && a->focal_x != 0.0 && a->focal_y != 0.0, SFGS_E_ARG,
               "SfgsDsmViewArgs: resolution %g, focal %g, %g", a->resolution, a->focal_x, a->focal_y);
  SFGS_REQUIRE(a->depth && acc && num_points, SFGS_E_ARG, "NULL argument");
  SFGS_REQUIRE(a->mode == SFGS_DSM_MAX || count, SFGS_E_ARG, "mean mode needs the count array");
  DsmView v;
  for (int i = 0; i < 9; ++i) v.cam.M[i] = a->M[i];
  for (int i = 0; i < 3; ++i) { v.cam.c[i] = a->c[i]; v.cam.origin[i] = a->origin[i]; }
  v.cam.cx_pix = a->cx_pix; v.cam.cy_pix = a->cy_pix; v.cam.focal_x = a->focal_x; v.cam.focal_y = a->focal_y;
  v.xoff = a->xoff; v.yoff_top = a->yoff_top; v.res = a->resolution;
  v.H = a->H; v.W = a->W; v.xsize = a->xsize; v.ysize = a->ysize; v.radius = a->radius;
  hipStream_t stream = (hipStream_t)stream_;
  const dim3 grid(geo_blocks((long long)a->H * a->W)), block(GEO_THREADS);
  if (a->mode == SFGS_DSM_MEAN)
    hipLaunchKernelGGL(dsm_accumulate_kernel<true>, grid, block, 0, stream, a->depth, a->mask, v, (unsigned long long*)acc, count,
                       num_points);
  else
    hipLaunchKernelGGL(dsm_accumulate_kernel<false>, grid, block, 0, stream, a->depth, a->mask, v, (unsigned long long*)acc, count,
                       num_points);
  SFGS_POST_LAUNCH("dsm_accumulate", stream, 0);
  return SFGS_OK;
}

extern "C" int sfgs_dsm_finalize(int32_t mode, int32_t xsize, int32_t ysize, const void* acc, const uint32_t* count, double* out,
                                 void* stream_) {
  if (const int rc = dsm_check_grid(xsize, ysize)) return rc;
  SFGS_REQUIRE(mode == SFGS_DSM_MAX || mode == SFGS_DSM_MEAN, SFGS_E_ARG, "sfgs_dsm_finalize: mode %d", mode);
  SFGS_REQUIRE(acc && out && (mode == SFGS_DSM_MAX || count), SFGS_E_ARG, "NULL argument");
  hipStream_t stream = (hipStream_t)stream_;
  const long long cells = (long long)xsize * ysize;
  const dim3 grid(geo_blocks(cells)), block(GEO_THREADS);
  if (mode == SFGS_DSM_MEAN)
    hipLaunchKernelGGL(dsm_finalize_kernel<true>, grid, block, 0, stream, (const unsigned long long*)acc, count, cells, out);
  else
    hipLaunchKernelGGL(dsm_finalize_kernel<false>, grid, block, 0, stream, (const unsigned long long*)acc, count, cells, out);
  SFGS_POST_LAUNCH("dsm_finalize", stream, 0);
  return SFGS_OK;
}

extern "C" size_t sfgs_dsmr_scratch_bytes(const SfgsDsmrArgs* args) {
  DsmrPlan p;
  return dsmr_plan(args, &p) == SFGS_OK ? p.total : 0;
}

extern "C" int sfgs_dsmr_register(const SfgsDsmrArgs* args, int32_t* shift_out, double* stats_out, void* scratch,
                                  size_t scratch_bytes, void* stream_) {
  DsmrPlan p;
  if (const int rc = dsmr_plan(args, &p)) return rc;
  SFGS_REQUIRE(shift_out && stats_out && scratch, SFGS_E_ARG, "NULL argument");
  SFGS_REQUIRE(scratch_bytes >= p.total, SFGS_E_CAPACITY, "dsmr scratch too small: %zu < %zu", scratch_bytes, p.total);
  hipStream_t stream = (hipStream_t)stream_;
  char* base = (char*)scratch;
  const double* u[GEO_MAX_LEVELS];
  const double* v[GEO_MAX_LEVELS];
  u[0] = args->ref; v[0] = args->sec;
  const dim3 block(GEO_THREADS);
  for (int k = 1; k < p.levels; ++k) {
    double* uk = (double*)(base + p.off_u[k]);
    double* vk = (double*)(base + p.off_v[k]);
    hipLaunchKernelGGL(dsmr_downsample_kernel, dim3(geo_blocks((long long)p.Hu[k] * p.Wu[k])), block, 0, stream, u[k - 1],
                       p.Hu[k - 1], p.Wu[k - 1], uk, p.Hu[k], p.Wu[k]);
    hipLaunchKernelGGL(dsmr_downsample_kernel, dim3(geo_blocks((long long)p.Hv[k] * p.Wv[k])), block, 0, stream, v[k - 1],
                       p.Hv[k - 1], p.Wv[k - 1], vk, p.Hv[k], p.Wv[k]);
    SFGS_POST_LAUNCH("dsmr_downsample", stream, 0);
    u[k] = uk; v[k] = vk;
  }
  // the start of the coarsest level: the caller's start halved (floor) once per level, as recursive_ncc does on its way down
  int dx = args->init_dx, dy = args->init_dy;
  for (int k = 1; k < p.levels; ++k) { dx = floordiv2(dx); dy = floordiv2(dy); }
  double* part = (double*)(base + p.off_part);
  double* mean = (double*)(base + p.off_mean);
  int* lshift = (int*)(base + p.off_shift);
  double* lstats = (double*)(base + p.off_stats);
  for (int k = p.levels - 1; k >= 0; --k) {
    DsmrLevel L;
    L.u = u[k]; L.v = v[k]; L.Hu = p.Hu[k]; L.Wu = p.Wu[k]; L.Hv = p.Hv[k]; L.Wv = p.Wv[k];
    L.irange = args->irange; L.init_dx = dx; L.init_dy = dy;
    L.below = k == p.levels - 1 ? nullptr : lshift + 2 * (k + 1);
    L.tiles_x = (L.Wu + GEO_TILE - 1) / GEO_TILE;
    L.tiles = L.tiles_x * ((L.Hu + GEO_TILE - 1) / GEO_TILE);
    int* so = k == 0 ? shift_out : lshift + 2 * k;
    double* st = k == 0 ? stats_out : lstats + 8 * k;
    hipLaunchKernelGGL(dsmr_tile_kernel<1>, dim3((unsigned)L.tiles), block, 0, stream, L, (const double*)mean, part);
    SFGS_POST_LAUNCH("dsmr_tile1", stream, 0);
    hipLaunchKernelGGL(dsmr_mean_kernel, dim3(1), block, 0, stream, (const double*)part, L.tiles, p.nshift, mean);
    SFGS_POST_LAUNCH("dsmr_mean", stream, 0);
    hipLaunchKernelGGL(dsmr_tile_kernel<2>, dim3((unsigned)L.tiles), block, 0, stream, L, (const double*)mean, part);
    SFGS_POST_LAUNCH("dsmr_tile2", stream, 0);
    hipLaunchKernelGGL(dsmr_select_kernel, dim3(1), block, 0, stream, L, (const double*)part, (const double*)mean,
                       args->scaling != 0 && k == 0, so, st);
    SFGS_POST_LAUNCH("dsmr_select", stream, 0);
  }
  return SFGS_OK;
}

extern "C" int sfgs_dsm_apply_shift(const double* sec, int32_t H, int32_t W, const int32_t* shift, const double* ab, double* out,
                                    void* stream_) {
  if (const int rc = geo_check_raster("sfgs_dsm_apply_shift", H, W)) return rc;
  SFGS_REQUIRE(sec && shift && ab && out, SFGS_E_ARG, "NULL argument");
  hipStream_t stream = (hipStream_t)stream_;
  hipLaunchKernelGGL(dsm_apply_shift_kernel, dim3(geo_blocks((long long)H * W)), dim3(GEO_THREADS), 0, stream, sec, H, W, shift,
                     ab, out);
  SFGS_POST_LAUNCH("dsm_apply_shift", stream, 0);
  return SFGS_OK;
}

extern "C" size_t sfgs_dsm_metrics_scratch_bytes(int32_t H, int32_t W) {
  if (geo_check_raster("sfgs_dsm_metrics", H, W)) return 0;
  return (size_t)5 * GEO_METRIC_MAX_BLOCKS * 8;
}

extern "C" int sfgs_dsm_metrics(const double* pred, const double* gt, const unsigned char* mask, int32_t H, int32_t W,
                                const int32_t* shift, const double* ab, double* out, void* scratch, size_t scratch_bytes,
                                void* stream_) {
  if (const int rc = geo_check_raster("sfgs_dsm_metrics", H, W)) return rc;
  SFGS_REQUIRE(pred && gt && out && scratch, SFGS_E_ARG, "NULL argument");
  SFGS_REQUIRE((shift == nullptr) == (ab == nullptr), SFGS_E_ARG, "sfgs_dsm_metrics: shift and ab come together");
  SFGS_REQUIRE(scratch_bytes >= (size_t)5 * GEO_METRIC_MAX_BLOCKS * 8, SFGS_E_CAPACITY, "dsm metrics scratch too small: %zu < %zu",
               scratch_bytes, (size_t)5 * GEO_METRIC_MAX_BLOCKS * 8);
  hipStream_t stream = (hipStream_t)stream_;
  const long long P = (long long)H * W;
  const unsigned want = geo_blocks(P);
  const int blocks = (int)(want < (unsigned)GEO_METRIC_MAX_BLOCKS ? want : (unsigned)GEO_METRIC_MAX_BLOCKS);
  hipLaunchKernelGGL(dsm_metrics_kernel, dim3((unsigned)blocks), dim3(GEO_THREADS), 0, stream, pred, gt, mask, H, W, shift, ab,
                     (double*)scratch);
  SFGS_POST_LAUNCH("dsm_metrics", stream, 0);
  hipLaunchKernelGGL(dsm_metrics_final_kernel, dim3(1), dim3(64), 0, stream, (const double*)scratch, blocks, out);
  SFGS_POST_LAUNCH("dsm_metrics_final", stream, 0);
  return SFGS_OK;
}
