// tsdf_raycast_check.cpp -- the ray-cast of the product's tsdf_math.h (skyfall-gs_amd/csrc) built with g++ for the CPU suite: the
// per-pixel function that tsdf_raycast_kernel runs, with both marches, and the empty-space table, driven by plain loops.
// tests/tsdf_raycast_hostcheck.py is the ctypes front-end; tests/test_tsdf_raycast_host.py holds the results to
// tests/tsdf_raycast_np.py byte for byte. Test infrastructure only.
#include <stdint.h>
#include <string.h>

#include "../../include/sfgs.h"
#include "../../skyfall-gs_amd/csrc/tsdf_math.h"

using namespace sfgs;

namespace {

TsdfRayGrid grid_of(const SfgsTsdfVolume& v) {
  TsdfRayGrid g;
  g.nx = v.nx; g.ny = v.ny; g.nz = v.nz;
  g.bx = tsdf_skip_bricks(v.nx); g.by = tsdf_skip_bricks(v.ny); g.bz = tsdf_skip_bricks(v.nz);
  for (int a = 0; a < 3; ++a) g.origin[a] = v.origin[a];
  g.voxel_size = v.voxel_size;
  g.inv_voxel = 1.0 / v.voxel_size;
  return g;
}

TsdfRayCamera camera_of(const SfgsTsdfRay& r) {
  TsdfRayCamera cam;
  for (int k = 0; k < 9; ++k) cam.M[k] = r.M[k];
  for (int k = 0; k < 3; ++k) cam.c[k] = r.c[k];
  cam.cx_pix = r.cx_pix; cam.cy_pix = r.cy_pix; cam.focal_x = r.focal_x; cam.focal_y = r.focal_y;
  cam.near = r.near; cam.far = r.far; cam.step = r.step;
  return cam;
}

template <bool COLORS, bool NORMALS, bool SKIP>
void raycast(const SfgsTsdfVolume& v, const SfgsTsdfRay& r, const unsigned char* skip, TsdfRayCounters* n) {
  const TsdfRayGrid g = grid_of(v);
  const TsdfRayCamera cam = camera_of(r);
  const long long P = (long long)r.H * r.W;
  for (int row = 0; row < r.H; ++row)
    for (int col = 0; col < r.W; ++col) {
      float depth, normal[3], colour[3];
      tsdf_ray_pixel<COLORS, NORMALS, SKIP>(g, cam, row, col, v.tsdf, v.weight, v.rgb, skip, &depth, normal, colour, n);
      const long long p = (long long)row * r.W + col;
      r.depth[p] = depth;
      for (int c = 0; c < 3; ++c) {
        if (NORMALS) r.normal[c * P + p] = normal[c];
        if (COLORS) r.rgb[c * P + p] = colour[c];
      }
    }
}

template <bool COLORS, bool NORMALS>
void raycast(const SfgsTsdfVolume& v, const SfgsTsdfRay& r, const unsigned char* skip, TsdfRayCounters* n) {
  if (skip) raycast<COLORS, NORMALS, true>(v, r, skip, n); else raycast<COLORS, NORMALS, false>(v, r, skip, n);
}

}  // namespace

// counters: int64 [4] that receives the samples evaluated, the jumps taken, the longest jump in lattice steps and the longest run
// of samples not evaluated.
// skip: the table (trc_skip_build) or NULL for the uniform march. A volume without cells: zeros, as the library writes them.
extern "C" int trc_raycast(const SfgsTsdfVolume* vol, const SfgsTsdfRay* ray, const unsigned char* skip, int64_t* counters) {
  if (!vol || !ray || !counters || !ray->depth || (vol->rgb != nullptr) != (ray->rgb != nullptr)) return -1;
  TsdfRayCounters n = {0, 0, 0, 0};
  const long long P = (long long)ray->H * ray->W;
  if (vol->nx < 2 || vol->ny < 2 || vol->nz < 2) {
    memset(ray->depth, 0, P * 4);
    if (ray->normal) memset(ray->normal, 0, P * 12);
    if (ray->rgb) memset(ray->rgb, 0, P * 12);
  } else if (ray->rgb) {
    if (ray->normal) raycast<true, true>(*vol, *ray, skip, &n); else raycast<true, false>(*vol, *ray, skip, &n);
  } else {
    if (ray->normal) raycast<false, true>(*vol, *ray, skip, &n); else raycast<false, false>(*vol, *ray, skip, &n);
  }
  counters[0] = n.samples; counters[1] = n.jumps; counters[2] = n.longest; counters[3] = n.longest_run;
  return 0;
}

// The table in tsdf_skip_kernel's terms: a byte per brick from tsdf_skip_flag over the brick's footprint.
extern "C" int trc_skip_build(const SfgsTsdfVolume* vol, unsigned char* skip, size_t bytes) {
  if (!vol || !skip) return -1;
  const TsdfRayGrid g = grid_of(*vol);
  if (bytes < (size_t)g.bx * g.by * g.bz) return -2;
  memset(skip, 0, (size_t)g.bx * g.by * g.bz);
  if (vol->nx < 2 || vol->ny < 2 || vol->nz < 2) return 0;
  const int n[3] = {g.nx, g.ny, g.nz};
  for (int bz = 0; bz < g.bz; ++bz)
    for (int by = 0; by < g.by; ++by)
      for (int bx = 0; bx < g.bx; ++bx) {
        const int b[3] = {bx, by, bz};
        int lo[3], hi[3];
        for (int a = 0; a < 3; ++a) {
          lo[a] = b[a] * TSDF_SKIP_BRICK;
          hi[a] = lo[a] + TSDF_SKIP_BRICK < n[a] - 1 ? lo[a] + TSDF_SKIP_BRICK : n[a] - 1;
        }
        bool any = false;
        for (int z = lo[2]; z <= hi[2]; ++z)
          for (int y = lo[1]; y <= hi[1]; ++y)
            for (int x = lo[0]; x <= hi[0]; ++x) {
              const long long p = ((long long)z * g.ny + y) * g.nx + x;
              any = any || tsdf_skip_flag(vol->weight[p], vol->tsdf[p]);
            }
        skip[((long long)bz * g.by + by) * g.bx + bx] = any ? 1 : 0;
      }
  return 0;
}
