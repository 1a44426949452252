// The host build of csrc/mesh_raster_math.h: the functions csrc/mesh_raster.hip runs per vertex, face and pixel, driven by plain
// sequential loops (tests/mesh_render_hostcheck.py binds this file with ctypes). Build: g++ -O2 -ffp-contract=off.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../skyfall-gs_amd/csrc/mesh_raster_math.h"

using namespace sfgs;

namespace {

GeoCamera camera_of(const double* cam) {        // M[9], c[3], cx_pix, cy_pix, focal_x, focal_y
  GeoCamera g;
  for (int k = 0; k < 9; ++k) g.M[k] = cam[k];
  for (int k = 0; k < 3; ++k) { g.c[k] = cam[9 + k]; g.origin[k] = 0.0; }
  g.cx_pix = cam[12]; g.cy_pix = cam[13]; g.focal_x = cam[14]; g.focal_y = cam[15];
  return g;
}

}  // namespace

extern "C" int mrc_camera_sign(const double* cam) { return mr_camera_sign(camera_of(cam)); }

// -> usable; X, Y, z of the record
extern "C" int mrc_project(const double* cam, const float* p, double near, int32_t* X, int32_t* Y, double* z) {
  const MrVertex r = mr_project(camera_of(cam), p, near);
  *X = r.X; *Y = r.Y; *z = r.z;
  return r.X != MR_UNUSABLE;
}

// corners as (X, Y) pairs with depth 1 -> the outcome; A and sgn when drawn
extern "C" int mrc_face(const int32_t* xy, int camera_sign, int cull, long long* A, int* sgn) {
  MrVertex v[3];
  for (int i = 0; i < 3; ++i) { v[i].X = xy[2 * i]; v[i].Y = xy[2 * i + 1]; v[i].z = 1.0; }
  MrFace f;
  const int outcome = mr_face_setup(v[0], v[1], v[2], camera_sign, cull, &f);
  *A = outcome == MR_DRAWN ? f.A : 0; *sgn = outcome == MR_DRAWN ? f.sgn : 0;
  return outcome;
}

// the three edge values of a drawn face at a pixel, whether each edge owns a zero, and the verdict
extern "C" int mrc_covers(const int32_t* xy, int col, int row, long long* E, int* owns) {
  MrVertex v[3];
  for (int i = 0; i < 3; ++i) { v[i].X = xy[2 * i]; v[i].Y = xy[2 * i + 1]; v[i].z = 1.0; }
  MrFace f;
  if (mr_face_setup(v[0], v[1], v[2], 1, 0, &f) != MR_DRAWN) return -1;
  for (int i = 0; i < 3; ++i) {
    long long dx, dy;
    mr_edge_dir(f, i, &dx, &dy);
    owns[i] = mr_edge_owns_zero(dx, dy);
  }
  return mr_covers(f, col, row, E);
}

// the whole view, face after face, pixel after pixel. vnormals: NULL = flat. normal / rgb: NULL = not wanted.
extern "C" int mrc_render(const double* cam, double near, double far, int cull, int H, int W, const float* vertices, const float* colors,
                          const int32_t* faces, const float* vnormals, long long m, long long n, float* depth, int32_t* face_out,
                          float* normal, float* rgb, long long* counts, int32_t* cover) {
  const GeoCamera g = camera_of(cam);
  const int camera_sign = mr_camera_sign(g);
  std::vector<MrVertex> rec((size_t)m);
  for (long long v = 0; v < m; ++v) rec[v] = mr_project(g, vertices + 3 * v, near);
  const long long P = (long long)H * W;
  std::vector<unsigned long long> keys((size_t)P, MR_EMPTY_KEY);
  for (int k = 0; k < 4; ++k) counts[k] = 0;
  int status = 0;
  for (long long t = 0; t < n; ++t) {
    const int32_t ia = faces[3 * t], ib = faces[3 * t + 1], ic = faces[3 * t + 2];
    if (!(mesh_index_ok(ia, m) && mesh_index_ok(ib, m) && mesh_index_ok(ic, m))) { counts[MR_CLIPPED]++; status |= MESH_ST_BAD_INDEX; continue; }
    MrFace f;
    const int outcome = mr_face_setup(rec[ia], rec[ib], rec[ic], camera_sign, cull, &f);
    counts[outcome]++;
    int c0, c1, r0, r1;
    if (outcome != MR_DRAWN || !mr_box(f, H, W, &c0, &c1, &r0, &r1)) continue;
    for (int row = r0; row <= r1; ++row)
      for (int col = c0; col <= c1; ++col) {
        long long E[3];
        if (!mr_covers(f, col, row, E)) continue;
        const long long p = (long long)row * W + col;
        cover[p]++;
        double q[3], s;
        const float d = mr_depth(f, E, q, &s);
        if (!mr_depth_kept(d, far)) continue;
        const unsigned long long key = mr_key(d, (uint32_t)t);
        if (key < keys[p]) keys[p] = key;
      }
  }
  for (long long p = 0; p < P; ++p) {
    float nrm[3] = {0.f, 0.f, 0.f}, c[3] = {0.f, 0.f, 0.f};
    depth[p] = 0.f; face_out[p] = -1;
    if (keys[p] != MR_EMPTY_KEY) {
      const uint32_t face = (uint32_t)keys[p];
      depth[p] = mr_key_depth(keys[p]); face_out[p] = (int32_t)face;
      mr_resolve_pixel(rec.data(), faces, vertices, rgb ? colors : nullptr, vnormals, camera_sign, face, (int)(p % W), (int)(p / W),
                       normal != nullptr, nrm, c);
    }
    for (int a = 0; a < 3; ++a) {
      if (normal) normal[a * P + p] = nrm[a];
      if (rgb) rgb[a * P + p] = c[a];
    }
  }
  return status;
}
