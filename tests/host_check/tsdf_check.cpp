// tsdf_check.cpp -- the product's tsdf_math.h (skyfall-gs_amd/csrc) built with g++ for the CPU suite: the per-voxel update and the
// per-cell triangulation that tsdf.hip runs on the device, driven by plain loops in the kernels' order. tests/tsdf_hostcheck.py
// is the ctypes front-end; tests/test_tsdf_host.py holds the results to tests/tsdf_np.py byte for byte. Test infrastructure only.
#include <stdint.h>
#include <string.h>

#include "../../include/sfgs.h"
#include "../../skyfall-gs_amd/csrc/tsdf_math.h"

using namespace sfgs;

namespace {

GeoCamera camera_of(const SfgsTsdfView& r) {
  GeoCamera g;
  for (int k = 0; k < 9; ++k) g.M[k] = r.M[k];
  for (int k = 0; k < 3; ++k) { g.c[k] = r.c[k]; g.origin[k] = 0.0; }
  g.cx_pix = r.cx_pix; g.cy_pix = r.cy_pix; g.focal_x = r.focal_x; g.focal_y = r.focal_y;
  return g;
}

template <bool COLORS>
void integrate(const SfgsTsdfVolume& v, const SfgsTsdfView* views, int V, int64_t* outcomes) {
  const long long nvox = (long long)v.nx * v.ny * v.nz;
  for (int k = 0; k < v.nz; ++k)
    for (int j = 0; j < v.ny; ++j)
      for (int i = 0; i < v.nx; ++i) {
        const long long p = ((long long)k * v.ny + j) * v.nx + i;
        const double centre[3] = {tsdf_centre(v.origin[0], i, v.voxel_size), tsdf_centre(v.origin[1], j, v.voxel_size),
                                  tsdf_centre(v.origin[2], k, v.voxel_size)};
        float D = v.tsdf[p], Wt = v.weight[p], col[3] = {0.f, 0.f, 0.f};
        if (COLORS)
          for (int c = 0; c < 3; ++c) col[c] = v.rgb[c * nvox + p];
        bool touched = false;
        for (int n = 0; n < V; ++n) {
          const TsdfOutcome o = tsdf_update<COLORS>(camera_of(views[n]), views[n].H, views[n].W, views[n].depth, views[n].mask,
                                                    views[n].image, centre, v.trunc, v.max_weight, &D, &Wt, col);
          if (outcomes) ++outcomes[(int)o];
          touched |= o == TSDF_UPDATED;
        }
        if (!touched) continue;
        v.tsdf[p] = D;
        v.weight[p] = Wt;
        if (COLORS)
          for (int c = 0; c < 3; ++c) v.rgb[c * nvox + p] = col[c];
      }
}

template <bool COLORS>
long long extract(const SfgsTsdfVolume& v, float* vertices, float* colors, long long capacity) {
  TsdfMeshFrame f;
  for (int a = 0; a < 3; ++a) f.origin[a] = (float)v.origin[a];
  f.voxel_size = (float)v.voxel_size;
  const long long plane = (long long)v.nx * v.ny, nvox = plane * v.nz;
  long long rows = 0;
  for (int z = 0; z + 1 < v.nz; ++z)
    for (int y = 0; y + 1 < v.ny; ++y)
      for (int x = 0; x + 1 < v.nx; ++x) {
        const long long base = ((long long)z * v.ny + y) * v.nx + x;
        float val[8], col[3][8];
        memset(col, 0, sizeof(col));
        bool used = true;
        for (int k = 0; k < 8; ++k) {
          const long long q = base + (k & 1) + (long long)((k >> 1) & 1) * v.nx + (long long)((k >> 2) & 1) * plane;
          used = used && v.weight[q] > 0.f;
          val[k] = v.tsdf[q];
          if (COLORS)
            for (int c = 0; c < 3; ++c) col[c][k] = v.rgb[c * nvox + q];
        }
        if (!used) continue;
        const int n = tsdf_cell_emit<COLORS>(f, val, col, x, y, z, vertices, colors, rows, capacity);
        if (n != tsdf_cell_count(val)) return -1;             // the count pass and the emit pass must agree
        rows += n;
      }
  return rows;
}

}  // namespace

// outcomes: NULL, or int64 [5] that receives how many (voxel, view) pairs ended as each TsdfOutcome
extern "C" int tc_integrate(const SfgsTsdfVolume* vol, const SfgsTsdfView* views, int32_t V, int64_t* outcomes) {
  if (!vol || !views || V < 1 || V > TSDF_MAX_VIEWS) return -1;
  if (outcomes) memset(outcomes, 0, 5 * sizeof(int64_t));
  if (vol->rgb) integrate<true>(*vol, views, V, outcomes); else integrate<false>(*vol, views, V, outcomes);
  return 0;
}

// -> the number of triangles (rows at or beyond capacity are counted, not written); -1: count and emit disagree
extern "C" long long tc_extract(const SfgsTsdfVolume* vol, float* vertices, float* colors, long long capacity) {
  if (!vol || !vertices || (vol->rgb != nullptr) != (colors != nullptr)) return -2;
  return vol->rgb ? extract<true>(*vol, vertices, colors, capacity) : extract<false>(*vol, vertices, colors, capacity);
}

extern "C" int tc_tet_corner(int t, int l) { return tsdf_tet_corner(t, l); }
extern "C" int tc_winding_swap(int t, int m) { return tsdf_winding_swap(t, m) ? 1 : 0; }
extern "C" int tc_tet_triangles(int m) { return tsdf_tet_triangles(m); }
