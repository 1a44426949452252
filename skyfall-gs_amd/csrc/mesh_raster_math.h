// mesh_raster_math.h -- what the mesh rasteriser (mesh_raster.hip) decides per vertex, per face and per pixel, written ONCE for the
// device and for the host build that tests/host_check/mesh_render_check.cpp drives sequentially; tests/mesh_render_np.py states the
// same sequences in numpy and both are held to it byte for byte. Coverage is decided in int64, the winner of a pixel by an
// integer minimum; float64 only where a value is formed (depth, weights, attributes), one rounded operation at a time: build
// with -ffp-contract=off, no fma. Nothing here touches memory but the words it is handed.
#pragma once
#include <math.h>
#include <stdint.h>

#include "geo_unproject.h"
#include "mesh_math.h"

namespace sfgs {

constexpr double MR_SNAP = 256.0;                       // sub-pixel steps per pixel: X = rint(256 u)
constexpr int MR_SNAP_SHIFT = 8;
constexpr double MR_GUARD = 268435456.0;                // 2^28: |X|, |Y| beyond it make a vertex unusable
constexpr int32_t MR_UNUSABLE = INT32_MIN;              // X of an unusable vertex's record (|X| <= 2^28 otherwise)
constexpr unsigned long long MR_EMPTY_KEY = ~0ull;      // a pixel no face covers
enum { MR_DRAWN = 0, MR_CULLED = 1, MR_CLIPPED = 2, MR_DEGENERATE = 3 };

// the 16-byte record of a projected vertex
struct MrVertex { int32_t X, Y; double z; };
static_assert(sizeof(MrVertex) == 16, "a vertex record is 16 bytes");

// a drawn face: the snapped corners, the depths, |twice the area| and the sign that orients the edge functions
struct MrFace { long long X[3], Y[3]; double z[3]; long long A; int sgn; };

GEO_FN bool mr_finite(double x) { return x - x == 0.0; }

// +1 / -1: the sign of focal_x focal_y det(M). With +1 (a proper rotation, positive focal lengths) a face whose normal
// (b - a) x (c - a) points toward the camera has NEGATIVE signed area in (column, row) coordinates: with a, b, c in the camera's
// frame n . a = det[a b c], the screen area has the sign of det[a b c] / (za zb zc) times that of focal_x focal_y, and facing means n . a < 0.
MESH_HD int mr_camera_sign(const GeoCamera& v) {          // (the host forms it once per call)
  const double* M = v.M;
  const double d0 = M[0] * (M[4] * M[8] - M[5] * M[7]);
  const double d1 = M[1] * (M[3] * M[8] - M[5] * M[6]);
  const double d2 = M[2] * (M[3] * M[7] - M[4] * M[6]);
  const double det = (d0 - d1) + d2;
  const bool neg = (det < 0.0) != ((v.focal_x < 0.0) != (v.focal_y < 0.0));
  return neg ? -1 : 1;
}

// 1. vertex: float32 position -> record. Unusable: u, v or z not finite, z <= near, |X| or |Y| > 2^28 (tested on the doubles).
GEO_FN MrVertex mr_project(const GeoCamera& cam, const float* p, double near) {
  const double w[3] = {(double)p[0], (double)p[1], (double)p[2]};
  double u, v, z;
  geo_project(cam, w, &u, &v, &z);
  MrVertex r;
  r.X = MR_UNUSABLE; r.Y = 0; r.z = 0.0;
  if (!(mr_finite(u) && mr_finite(v) && mr_finite(z)) || z <= near) return r;
  const double xd = rint(u * MR_SNAP), yd = rint(v * MR_SNAP);
  if (!(fabs(xd) <= MR_GUARD && fabs(yd) <= MR_GUARD)) return r;
  r.X = (int32_t)xd; r.Y = (int32_t)yd; r.z = z;
  return r;
}

// 2. face: -> MR_DRAWN (f is filled), MR_CLIPPED, MR_DEGENERATE or MR_CULLED. cull != 0: faces turned away are not drawn.
GEO_FN int mr_face_setup(const MrVertex& a, const MrVertex& b, const MrVertex& c, int camera_sign, int cull, MrFace* f) {
  if (a.X == MR_UNUSABLE || b.X == MR_UNUSABLE || c.X == MR_UNUSABLE) return MR_CLIPPED;
  f->X[0] = a.X; f->X[1] = b.X; f->X[2] = c.X;
  f->Y[0] = a.Y; f->Y[1] = b.Y; f->Y[2] = c.Y;
  f->z[0] = a.z; f->z[1] = b.z; f->z[2] = c.z;
  const long long As = (f->X[1] - f->X[0]) * (f->Y[2] - f->Y[0]) - (f->Y[1] - f->Y[0]) * (f->X[2] - f->X[0]);
  if (As == 0) return MR_DEGENERATE;
  const bool facing = (As < 0) == (camera_sign > 0);
  if (cull && !facing) return MR_CULLED;
  f->sgn = As < 0 ? -1 : 1;
  f->A = As < 0 ? -As : As;
  return MR_DRAWN;
}

// the face's box of pixels clipped to the image; false: it holds no pixel. floor and ceil of X / 256 by arithmetic shifts.
GEO_FN bool mr_box(const MrFace& f, int H, int W, int* c0, int* c1, int* r0, int* r1) {
  long long x0 = f.X[0], x1 = f.X[0], y0 = f.Y[0], y1 = f.Y[0];
  for (int i = 1; i < 3; ++i) {
    x0 = f.X[i] < x0 ? f.X[i] : x0; x1 = f.X[i] > x1 ? f.X[i] : x1;
    y0 = f.Y[i] < y0 ? f.Y[i] : y0; y1 = f.Y[i] > y1 ? f.Y[i] : y1;
  }
  long long ca = (x0 + 255) >> MR_SNAP_SHIFT, cb = x1 >> MR_SNAP_SHIFT, ra = (y0 + 255) >> MR_SNAP_SHIFT, rb = y1 >> MR_SNAP_SHIFT;
  if (ca < 0) ca = 0;
  if (ra < 0) ra = 0;
  if (cb > W - 1) cb = W - 1;
  if (rb > H - 1) rb = H - 1;
  *c0 = (int)ca; *c1 = (int)cb; *r0 = (int)ra; *r1 = (int)rb;
  return ca <= cb && ra <= rb;
}

// 3. the edge opposite corner i, from corner j = i + 1 to k = i + 2 (mod 3), oriented so that the inside is positive:
// its direction (dx, dy) and its value at pixel (col, row). Inside the face's box every product stays below 2^59.
GEO_FN void mr_edge_dir(const MrFace& f, int i, long long* dx, long long* dy) {
  const int j = i == 2 ? 0 : i + 1, k = i == 0 ? 2 : i - 1;
  *dx = f.sgn * (f.X[k] - f.X[j]);
  *dy = f.sgn * (f.Y[k] - f.Y[j]);
}
GEO_FN long long mr_edge_at(const MrFace& f, int i, int col, int row) {
  const int j = i == 2 ? 0 : i + 1;
  long long dx, dy;
  mr_edge_dir(f, i, &dx, &dy);
  return dx * (((long long)row << MR_SNAP_SHIFT) - f.Y[j]) - dy * (((long long)col << MR_SNAP_SHIFT) - f.X[j]);
}
// a zero counts as inside for a left edge (it runs upward: dy < 0) and for a top edge (dy == 0, it runs to the right): a rule of
// the direction alone that answers the two directions of one edge differently
GEO_FN bool mr_edge_owns_zero(long long dx, long long dy) { return dy < 0 || (dy == 0 && dx > 0); }
GEO_FN bool mr_edge_inside(long long E, long long dx, long long dy) { return E > 0 || (E == 0 && mr_edge_owns_zero(dx, dy)); }

GEO_FN bool mr_covers(const MrFace& f, int col, int row, long long* E) {
  bool in = true;
  for (int i = 0; i < 3; ++i) {
    long long dx, dy;
    mr_edge_dir(f, i, &dx, &dy);
    E[i] = mr_edge_at(f, i, col, row);
    in = in && mr_edge_inside(E[i], dx, dy);
  }
  return in;
}

// 4. depth of a covered pixel from its three edge values; q and s are what the attributes use
GEO_FN float mr_depth(const MrFace& f, const long long* E, double* q, double* s) {
  q[0] = (double)E[0] / f.z[0]; q[1] = (double)E[1] / f.z[1]; q[2] = (double)E[2] / f.z[2];
  *s = (q[0] + q[1]) + q[2];
  return (float)((double)f.A / *s);
}
GEO_FN bool mr_depth_kept(float d, double far) { return d > 0.f && (double)d <= far; }

// 5. the key whose minimum wins the pixel
GEO_FN unsigned long long mr_key(float depth, uint32_t face) {
  union { float f; uint32_t u; } b;
  b.f = depth;
  return ((unsigned long long)b.u << 32) | face;
}
GEO_FN float mr_key_depth(unsigned long long key) {
  union { float f; uint32_t u; } b;
  b.u = (uint32_t)(key >> 32);
  return b.f;
}

// 6. an attribute from the corners' float32 values
GEO_FN double mr_interp(const double* q, double s, float a0, float a1, float a2) {
  const double b0 = q[0] / s, b1 = q[1] / s, b2 = q[2] / s;
  return (b0 * (double)a0 + b1 * (double)a1) + b2 * (double)a2;
}

// everything of one winning pixel but its depth: the face's records again, the weights, normal and colour.
// vnormals: NULL = the flat normal. want_normal / colors: which outputs are formed.
GEO_FN void mr_resolve_pixel(const MrVertex* rec, const int32_t* faces, const float* vertices, const float* colors,
                             const float* vnormals, int camera_sign, uint32_t face, int col, int row, bool want_normal,
                             float* normal, float* rgb) {
  const int32_t ia = faces[3 * (long long)face], ib = faces[3 * (long long)face + 1], ic = faces[3 * (long long)face + 2];
  MrFace f = MrFace();
  mr_face_setup(rec[ia], rec[ib], rec[ic], camera_sign, 0, &f);      // a winner was drawn: its set-up succeeds again
  long long E[3];
  mr_covers(f, col, row, E);
  double q[3], s;
  mr_depth(f, E, q, &s);
  if (want_normal) {
    double N[3];
    if (vnormals) {
      for (int a = 0; a < 3; ++a) N[a] = mr_interp(q, s, vnormals[3 * (long long)ia + a], vnormals[3 * (long long)ib + a], vnormals[3 * (long long)ic + a]);
    } else {
      mesh_face_normal(vertices + 3 * (long long)ia, vertices + 3 * (long long)ib, vertices + 3 * (long long)ic, N);
    }
    mesh_normalize(N, normal);
  }
  if (colors) {
    for (int a = 0; a < 3; ++a)
      rgb[a] = (float)mr_interp(q, s, colors[3 * (long long)ia + a], colors[3 * (long long)ib + a], colors[3 * (long long)ic + a]);
  }
}

}  // namespace sfgs
