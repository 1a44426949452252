// consistency.hip -- multi-view depth consistency: which pixels of a depth map do enough OTHER views confirm? The mask the
// geometry products (geometry.hip, pointcloud.hip, ortho.hip) take per view and nothing produced so far. The reference has no
// such step; the pair test is the geometric check of multi-view stereo fusion, stated in include/sfgs.h and, in numpy, in
// tests/consistency_np.py; this file is held to that restatement bit for bit.
//   cons_check_kernel, one launch per reference view i: a thread per reference pixel. The pixel is unprojected once
//   (geo_unproject.h: geometry.hip's float64 sequence) and then walks the sources j != i in ascending order:
//     project into j (geo_project) -> nearest pixel, range-checked on the doubles -> its depth, if used -> depth test ->
//     unproject THAT pixel of j, project it back into i -> distance from the pixel we started at.
//   Every accepted source adds 1 to the pixel's count; keep = count >= min_views. A rejected pair leaves at its first failed test.
// Layout: a workgroup is a 16 x 16 pixel tile, a wave an 8 x 8 quarter of it, so that the 64 gathers of a wave fall into a
// window of the source map a few lines of 128 bytes high. The row-major run of 256 pixels per workgroup gathers along a line
// 64 pixels long and is 6.9 % slower on 24 views of 1024 x 1024 (profiles/r21_consistency_ab.txt). The source loop is
// uniform across the wave: the record of source j -- pointers, size, camera -- comes from the device table by scalar loads.
// No atomics of any kind, no shared words, no barrier: a pixel's two bytes are written by its own thread.
// Every index is range-checked before it is used: the reference pixel against its view's H x W before its load, the source
// pixel against the source's H x W (on the doubles, before the conversion) before its load. No profiler ids.
#include "sfgs_internal.h"
#include "geo_unproject.h"

#include <math.h>

namespace sfgs {

constexpr int CONS_TILE = 16;                      // a workgroup's tile is CONS_TILE x CONS_TILE pixels ...
constexpr int CONS_THREADS = CONS_TILE * CONS_TILE;
constexpr int CONS_WAVE_TILE = 8;                  // ... a wave's CONS_WAVE_TILE x CONS_WAVE_TILE
constexpr int CONS_MAX_VIEWS = 256;                // a count fits a byte: at most 255 sources

// the table's record as the kernel reads it: the layout of SfgsConsistencyView (checked below), origin implied zero
struct ConsView {
  const float* depth;
  const unsigned char* mask;
  int H, W;
  double M[9], c[3];
  double cx_pix, cy_pix, focal_x, focal_y;
};
static_assert(sizeof(ConsView) == sizeof(SfgsConsistencyView), "ConsView is SfgsConsistencyView");
static_assert(offsetof(ConsView, H) == offsetof(SfgsConsistencyView, H) && offsetof(ConsView, M) == offsetof(SfgsConsistencyView, M) &&
              offsetof(ConsView, c) == offsetof(SfgsConsistencyView, c) &&
              offsetof(ConsView, cx_pix) == offsetof(SfgsConsistencyView, cx_pix) &&
              offsetof(ConsView, focal_y) == offsetof(SfgsConsistencyView, focal_y), "ConsView is SfgsConsistencyView");

__device__ __forceinline__ GeoCamera cons_camera(const ConsView& r) {
  GeoCamera g;
#pragma unroll
  for (int k = 0; k < 9; ++k) g.M[k] = r.M[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) { g.c[k] = r.c[k]; g.origin[k] = 0.0; }
  g.cx_pix = r.cx_pix; g.cy_pix = r.cy_pix; g.focal_x = r.focal_x; g.focal_y = r.focal_y;
  return g;
}

__global__ void __launch_bounds__(CONS_THREADS)
cons_check_kernel(const ConsView* __restrict__ table, int V, int ref, int H, int W, double rel_tol, double px_tol2,
                  unsigned min_views, unsigned char* __restrict__ count, unsigned char* __restrict__ keep) {
  const ConsView& R = table[ref];
  if (R.H != H || R.W != W) return;                // the grid and the two outputs were sized by the caller's H, W: uniform exit
  const int tiles_x = (W + CONS_TILE - 1) / CONS_TILE;
  const int tile_y = (int)(blockIdx.x / (unsigned)tiles_x), tile_x = (int)(blockIdx.x - (unsigned)tile_y * (unsigned)tiles_x);
  const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const int col = tile_x * CONS_TILE + (int)(wave & 1u) * CONS_WAVE_TILE + (int)(lane & 7u);
  const int row = tile_y * CONS_TILE + (int)(wave >> 1) * CONS_WAVE_TILE + (int)(lane >> 3);
  if (row >= H || col >= W) return;                // no barrier follows
  const long long p = (long long)row * W + col;
  unsigned n = 0;
  float d;
  if (geo_pixel_used(R.depth, R.mask, p, &d)) {
    const GeoCamera rc = cons_camera(R);
    double w[3];
    geo_unproject(rc, row, col, d, w);
    for (int j = 0; j < V; ++j) {                  // uniform: j and the record are the same in every lane
      if (j == ref) continue;
      const ConsView& S = table[j];
      const GeoCamera sc = cons_camera(S);
      double u, v, z;
      geo_project(sc, w, &u, &v, &z);
      if (!(z > 0.0)) continue;                    // behind the source (NaN too)
      const double fu = floor(u + 0.5), fv = floor(v + 0.5);
      if (!(fu >= 0.0 && fu < (double)S.W && fv >= 0.0 && fv < (double)S.H)) continue;   // outside its image (NaN too)
      const int su = (int)fu, sv = (int)fv;        // in range: the doubles were tested
      float dj;
      if (!geo_pixel_used(S.depth, S.mask, (long long)sv * S.W + su, &dj)) continue;
      if (!(fabs((double)dj - z) <= rel_tol * z)) continue;
      double w2[3], u2, v2, z2;
      geo_unproject(sc, sv, su, dj, w2);
      geo_project(rc, w2, &u2, &v2, &z2);
      if (!(z2 > 0.0)) continue;
      const double du = u2 - (double)col, dv = v2 - (double)row;
      if (!(du * du + dv * dv <= px_tol2)) continue;
      ++n;                                         // <= V - 1 <= 255
    }
  }
  count[p] = (unsigned char)n;
  keep[p] = n >= min_views ? 1 : 0;
}

}  // namespace sfgs

using namespace sfgs;

extern "C" int sfgs_consistency_table_check(const SfgsConsistencyView* views, int32_t V) {
  SFGS_REQUIRE(views, SFGS_E_ARG, "NULL SfgsConsistencyView table");
  SFGS_REQUIRE(V >= 2 && V <= CONS_MAX_VIEWS, SFGS_E_ARG, "consistency: %d views, 2 ... %d", V, CONS_MAX_VIEWS);
  for (int k = 0; k < V; ++k) {
    const SfgsConsistencyView& r = views[k];
    SFGS_REQUIRE(r.H > 0 && r.W > 0, SFGS_E_ARG, "SfgsConsistencyView %d: H %d, W %d", k, r.H, r.W);
    SFGS_REQUIRE((long long)r.H * r.W <= (1ll << 30), SFGS_E_ARG, "SfgsConsistencyView %d: H * W must not exceed 2^30, got %d x %d", k,
                 r.H, r.W);
    SFGS_REQUIRE(r.depth, SFGS_E_ARG, "SfgsConsistencyView %d: NULL depth", k);
    SFGS_REQUIRE(r.focal_x != 0.0 && r.focal_y != 0.0, SFGS_E_ARG, "SfgsConsistencyView %d: focal %g, %g", k, r.focal_x, r.focal_y);
  }
  return SFGS_OK;
}

extern "C" int sfgs_consistency_check(const SfgsConsistencyArgs* a, unsigned char* count, unsigned char* keep, void* stream_) {
  SFGS_REQUIRE(a, SFGS_E_ARG, "NULL SfgsConsistencyArgs");
  SFGS_REQUIRE(a->struct_size == sizeof(SfgsConsistencyArgs), SFGS_E_ARG, "SfgsConsistencyArgs.struct_size %u, expected %zu",
               a->struct_size, sizeof(SfgsConsistencyArgs));
  SFGS_REQUIRE(a->V >= 2 && a->V <= CONS_MAX_VIEWS, SFGS_E_ARG, "SfgsConsistencyArgs.V %d: 2 ... %d", a->V, CONS_MAX_VIEWS);
  SFGS_REQUIRE(a->ref >= 0 && a->ref < a->V, SFGS_E_ARG, "SfgsConsistencyArgs.ref %d: 0 ... %d", a->ref, a->V - 1);
  SFGS_REQUIRE(a->H > 0 && a->W > 0, SFGS_E_ARG, "SfgsConsistencyArgs: H %d, W %d", a->H, a->W);
  SFGS_REQUIRE((long long)a->H * a->W <= (1ll << 30), SFGS_E_ARG, "SfgsConsistencyArgs: H * W must not exceed 2^30, got %d x %d", a->H,
               a->W);
  SFGS_REQUIRE(a->rel_tol > 0.0 && a->rel_tol < INFINITY, SFGS_E_ARG, "SfgsConsistencyArgs.rel_tol %g: finite and > 0", a->rel_tol);
  SFGS_REQUIRE(a->px_tol2 > 0.0, SFGS_E_ARG, "SfgsConsistencyArgs.px_tol2 %g: > 0 (+inf: no bound)", a->px_tol2);
  SFGS_REQUIRE(a->min_views >= 1, SFGS_E_ARG, "SfgsConsistencyArgs.min_views %d: >= 1", a->min_views);
  SFGS_REQUIRE(a->table && count && keep, SFGS_E_ARG, "NULL argument");
  hipStream_t stream = (hipStream_t)stream_;
  const long long tiles = (long long)((a->W + CONS_TILE - 1) / CONS_TILE) * ((a->H + CONS_TILE - 1) / CONS_TILE);   // <= 2^26
  hipLaunchKernelGGL(cons_check_kernel, dim3((unsigned)tiles), dim3(CONS_THREADS), 0, stream, (const ConsView*)a->table, a->V,
                     a->ref, a->H, a->W, a->rel_tol, a->px_tol2, (unsigned)a->min_views, count, keep);
  SFGS_POST_LAUNCH("cons_check", stream, 0);
  return SFGS_OK;
}
