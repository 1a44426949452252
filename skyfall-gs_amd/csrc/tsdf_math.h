// tsdf_math.h -- the per-voxel update of TSDF fusion, the per-cell marching-tetrahedra triangulation and the per-pixel ray-cast,
// written ONCE: tsdf.hip runs them on the device, tests/host_check/tsdf_check.cpp and tsdf_raycast_check.cpp build them with g++
// for the CPU suite (GEO_FN: geo_unproject.h), and tests/tsdf_np.py and tests/tsdf_raycast_np.py state them in numpy; the three
// are held to each other byte for byte. include/sfgs.h gives the sequences in words. Nothing is contracted (-ffp-contract=off on
// both compilers): products, sums and quotients in the order written.
#pragma once
#include "geo_unproject.h"

namespace sfgs {

constexpr int TSDF_MAX_VIEWS = 256;      // views per integrate call

// The outcome of one (voxel, view) pair; the first four leave the voxel as it was.
enum TsdfOutcome { TSDF_BEHIND = 0, TSDF_OUTSIDE, TSDF_UNUSED, TSDF_BEYOND_TRUNC, TSDF_UPDATED };

// Centre of voxel i along one axis, in float64 as written.
GEO_FN double tsdf_centre(double origin, int i, double voxel_size) { return origin + ((double)i + 0.5) * voxel_size; }

// Running mean of a stored float32 value: float32((W * old + x) / (W + 1)), in float64.
GEO_FN float tsdf_mean(double Wd, float old, double x) { return (float)((Wd * (double)old + x) / (Wd + 1.0)); }

// One view into one voxel. The voxel's state (D, Wt and, with COLORS, rgb) lives with the caller, in registers on the device.
// depth / mask / image: the view's [H][W], [H][W] and [3][H][W]. Every index is range-checked before its load: the pixel on the
// doubles before the conversion.
template <bool COLORS>
GEO_FN TsdfOutcome tsdf_update(const GeoCamera& cam, int H, int W, const float* __restrict__ depth,
                               const unsigned char* __restrict__ mask, const float* __restrict__ image, const double (&centre)[3],
                               double trunc, double max_weight, float* D, float* Wt, float (&rgb)[3]) {
  double u, v, z;
  geo_project(cam, centre, &u, &v, &z);
  if (!(z > 0.0)) return TSDF_BEHIND;                                   // NaN too
  const double fu = floor(u + 0.5), fv = floor(v + 0.5);
  if (!(fu >= 0.0 && fu < (double)W && fv >= 0.0 && fv < (double)H)) return TSDF_OUTSIDE;   // NaN too
  const long long p = (long long)(int)fv * W + (int)fu;                 // in range: the doubles were tested
  float d;
  if (!geo_pixel_used(depth, mask, p, &d)) return TSDF_UNUSED;
  const double sdf = (double)d - z;
  if (sdf < -trunc) return TSDF_BEYOND_TRUNC;
  double s = sdf / trunc;
  if (!(s < 1.0)) s = 1.0;
  const double Wd = (double)*Wt;
  *D = tsdf_mean(Wd, *D, s);
  if (COLORS) {
    const long long P = (long long)H * W;
    GEO_UNROLL
    for (int c = 0; c < 3; ++c) rgb[c] = tsdf_mean(Wd, rgb[c], (double)image[(long long)c * P + p]);
  }
  const double Wn = Wd + 1.0;
  *Wt = (float)(Wn < max_weight ? Wn : max_weight);
  return TSDF_UPDATED;
}

// ---- marching tetrahedra ---------------------------------------------------------------------------------------------------------
// Corner k of a cell has the offsets (k & 1, (k >> 1) & 1, (k >> 2) & 1) along x, y, z. The six tetrahedra are the paths
// (0, 1 << a, (1 << a) | (1 << b), 7) over the permutations (a, b, c) of (0, 1, 2) in lexicographic order:
//   (0,1,3,7) (0,1,5,7) (0,2,3,7) (0,2,6,7) (0,4,5,7) (0,4,6,7)
// Corner numbers ascend along a path, and so do the linear voxel indices: local vertex l < m means `l is the canonical first end`.
GEO_FN int tsdf_tet_corner(int t, int l) {
  // the two middle corners of path t, three bits each: 1,3  1,5  2,3  2,6  4,5  4,6
  const unsigned long long mid = 0x19ull | 0x29ull << 6 | 0x1Aull << 12 | 0x32ull << 18 | 0x2Cull << 24 | 0x34ull << 30;
  return l == 0 ? 0 : l == 3 ? 7 : (int)((mid >> (6 * t + 3 * (l - 1))) & 7ull);
}

// Swap the last two vertices of the triangles of (tetrahedron t, inside mask m) so that (b - a) x (c - a) points to the outside?
// Bit m of row t. tests/test_tsdf_host.py derives the 6 x 14 mixed cases from geometry and compares.
GEO_FN bool tsdf_winding_swap(int t, int m) {
  const unsigned rows01 = 0x4D24u | 0x32DAu << 16, rows23 = 0x32DAu | 0x4D24u << 16, rows45 = 0x4D24u | 0x32DAu << 16;
  const unsigned r = t < 2 ? rows01 : t < 4 ? rows23 : rows45;
  return ((r >> (16 * (t & 1) + m)) & 1u) != 0;
}

// Triangles of a tetrahedron with inside mask m (bit l: local vertex l has a value below 0): 0, 1 or 2.
GEO_FN int tsdf_tet_triangles(int m) {
  // per mask two bits: 0 for 0000 and 1111, 2 for the six masks with two bits set, 1 otherwise
  return (int)((0x16696994u >> (2 * m)) & 3u);
}

// Index of the lowest set bit of a four-bit mask (3 for an empty one: never used then).
GEO_FN int tsdf_low_bit(int m) { return (m & 1) ? 0 : (m & 2) ? 1 : (m & 4) ? 2 : 3; }

GEO_FN int tsdf_inside_mask(const float (&val)[8], int t) {
  int m = 0;
  GEO_UNROLL
  for (int l = 0; l < 4; ++l) m |= (val[tsdf_tet_corner(t, l)] < 0.f ? 1 : 0) << l;
  return m;
}

// Triangles of a USED cell (the caller tested the eight weights).
GEO_FN int tsdf_cell_count(const float (&val)[8]) {
  int n = 0;
  GEO_UNROLL
  for (int t = 0; t < 6; ++t) n += tsdf_tet_triangles(tsdf_inside_mask(val, t));
  return n;
}

// a[k] by selects: a run-time index would move the caller's eight registers to scratch memory on the device.
GEO_FN float tsdf_pick(const float (&a)[8], int k) {
  const float a01 = (k & 1) ? a[1] : a[0], a23 = (k & 1) ? a[3] : a[2], a45 = (k & 1) ? a[5] : a[4], a67 = (k & 1) ? a[7] : a[6];
  const float lo = (k & 2) ? a23 : a01, hi = (k & 2) ? a67 : a45;
  return (k & 4) ? hi : lo;
}

// The grid as the triangulation sees it: everything in float32.
struct TsdfMeshFrame {
  float origin[3], voxel_size;
};

// The point where the surface cuts the edge between local vertices la < lb of tetrahedron t in cell (x, y, z), float32 as written:
// t = va / (va - vb), pos = pa + t * (pb - pa) in voxel-index units, world = origin + (pos + 0.5) * voxel_size; colour by the same t.
template <bool COLORS>
GEO_FN void tsdf_edge_point(const TsdfMeshFrame& f, const float (&val)[8], const float (&col)[3][8], int t, int la, int lb, int x, int y,
                            int z, float (&out)[3], float (&out_col)[3]) {
  const int ka = tsdf_tet_corner(t, la), kb = tsdf_tet_corner(t, lb);
  const float va = tsdf_pick(val, ka), vb = tsdf_pick(val, kb);
  const float w = va / (va - vb);
  const int cell[3] = {x, y, z};
  GEO_UNROLL
  for (int a = 0; a < 3; ++a) {
    const float pa = (float)(cell[a] + ((ka >> a) & 1)), pb = (float)(cell[a] + ((kb >> a) & 1));
    const float step = w * (pb - pa);
    const float pos = pa + step;
    const float scaled = (pos + 0.5f) * f.voxel_size;
    out[a] = f.origin[a] + scaled;
  }
  if (COLORS) {
    GEO_UNROLL
    for (int c = 0; c < 3; ++c) {
      const float ca = tsdf_pick(col[c], ka), cb = tsdf_pick(col[c], kb);
      const float step = w * (cb - ca);
      out_col[c] = ca + step;
    }
  }
}

// The triangles of tetrahedron t of a used cell -> rows first, first + 1, ... of vertices (and colors), nine floats each; a row at
// or beyond `capacity` is not written. Returns the number of triangles (0, 1, 2) whether written or not.
//   one inside, vertex i:            the edge points (i, j), j ascending
//   three inside, outside vertex o:  the edge points (i, o), i ascending
//   two inside, i0 < i1, o0 < o1:    q0 = (i0, o0), q1 = (i0, o1), q2 = (i1, o1), q3 = (i1, o0): (q0, q1, q2) and (q0, q2, q3)
// then the last two vertices swapped where tsdf_winding_swap says so. An edge point takes its ends in canonical order whichever
// of them is inside, so every tetrahedron that shares the edge produces the same bytes.
template <bool COLORS>
GEO_FN int tsdf_tet_emit(const TsdfMeshFrame& f, const float (&val)[8], const float (&col)[3][8], int t, int x, int y, int z,
                         float* __restrict__ vertices, float* __restrict__ colors, long long first, long long capacity) {
  const int m = tsdf_inside_mask(val, t);
  const int n = tsdf_tet_triangles(m);
  if (n == 0) return 0;
  // the set bits of m and of its complement, ascending; every index below is static once the loops are unrolled
  const int mi1 = m & (m - 1), mo = ~m & 15, mo1 = mo & (mo - 1);
  const int i0 = tsdf_low_bit(m), i1 = tsdf_low_bit(mi1), i2 = tsdf_low_bit(mi1 & (mi1 - 1));
  const int o0 = tsdf_low_bit(mo), o1 = tsdf_low_bit(mo1), o2 = tsdf_low_bit(mo1 & (mo1 - 1));
  const bool one = mi1 == 0, three = mo1 == 0;                            // else two and two
  const int e[4][2] = {{i0, o0}, {one ? i0 : three ? i1 : i0, one ? o1 : three ? o0 : o1},
                       {one ? i0 : three ? i2 : i1, one ? o2 : three ? o0 : o1}, {i1, o0}};   // q0 ... q3 (q3: a quad only)
  float q[4][3], qc[4][3];
  GEO_UNROLL
  for (int j = 0; j < 4; ++j) {
    if (j < 3 || n == 2) {
      const int la = e[j][0] < e[j][1] ? e[j][0] : e[j][1], lb = e[j][0] < e[j][1] ? e[j][1] : e[j][0];
      tsdf_edge_point<COLORS>(f, val, col, t, la, lb, x, y, z, q[j], qc[j]);
    } else {
      GEO_UNROLL
      for (int a = 0; a < 3; ++a) q[j][a] = qc[j][a] = 0.f;
    }
  }
  const bool swap = tsdf_winding_swap(t, m);
  GEO_UNROLL
  for (int k = 0; k < 2; ++k) {
    if (k < n && first + k < capacity) {
      float* __restrict__ row = vertices + (first + k) * 9;
      GEO_UNROLL
      for (int a = 0; a < 3; ++a) {
        row[a] = q[0][a];
        row[3 + a] = swap ? q[k + 2][a] : q[k + 1][a];
        row[6 + a] = swap ? q[k + 1][a] : q[k + 2][a];
      }
      if (COLORS) {
        float* __restrict__ crow = colors + (first + k) * 9;
        GEO_UNROLL
        for (int a = 0; a < 3; ++a) {
          crow[a] = qc[0][a];
          crow[3 + a] = swap ? qc[k + 2][a] : qc[k + 1][a];
          crow[6 + a] = swap ? qc[k + 1][a] : qc[k + 2][a];
        }
      }
    }
  }
  return n;
}

// All triangles of a used cell, tetrahedron after tetrahedron. Returns their number.
template <bool COLORS>
GEO_FN int tsdf_cell_emit(const TsdfMeshFrame& f, const float (&val)[8], const float (&col)[3][8], int x, int y, int z,
                          float* __restrict__ vertices, float* __restrict__ colors, long long first, long long capacity) {
  int n = 0;
  GEO_UNROLL
  for (int t = 0; t < 6; ++t) n += tsdf_tet_emit<COLORS>(f, val, col, t, x, y, z, vertices, colors, first + n, capacity);
  return n;
}

// ---- ray-casting -----------------------------------------------------------------------------------------------------------------
// A camera ray marched through the volume on a lattice of depths; the first sign change from >= 0 to < 0 between two valid samples
// is the surface. include/sfgs.h states the sequence in words, tests/tsdf_raycast_np.py in numpy (the uniform march only);
// tsdf_raycast_kernel and tests/host_check/tsdf_raycast_check.cpp run the functions below. Float64 on the stored float32 values.
constexpr int TSDF_RAY_MAX_SAMPLES = 1 << 20;   // samples per ray
constexpr int TSDF_SKIP_BRICK = 8;              // cells per axis of a brick of the empty-space table

struct TsdfRayGrid {
  int nx, ny, nz;                               // every one >= 2: the caller launches nothing otherwise
  int bx, by, bz;                               // bricks per axis: tsdf_skip_bricks(n)
  double origin[3], voxel_size, inv_voxel;      // inv_voxel = 1.0 / voxel_size, formed once on the host
};

struct TsdfRayCamera {
  double M[9], c[3];
  double cx_pix, cy_pix, focal_x, focal_y, near, far, step;
};

// What the host build counts; the kernel passes nullptr.
struct TsdfRayCounters {
  long long samples;                            // samples whose eight corners were loaded
  long long jumps;                              // accepted jumps
  long long longest;                            // lattice steps of the longest one (it stays in one brick)
  long long longest_run;                        // most consecutive samples of a ray not evaluated: jumps and single steps, brick after brick
};

// constexpr: the host's launch code calls it too
constexpr int tsdf_skip_bricks(int n) { return n < 2 ? 1 : (n - 1 + TSDF_SKIP_BRICK - 1) / TSDF_SKIP_BRICK; }

// A voxel that sets its bricks' bytes: observed and inside.
GEO_FN bool tsdf_skip_flag(float weight, float value) { return weight > 0.f && value < 0.f; }

GEO_FN double tsdf_lerp(double a, double b, double f) { return a + f * (b - a); }

// Direction of pixel (row, col): the point at depth z along the forward axis is c + z * d.
GEO_FN void tsdf_ray_direction(const TsdfRayCamera& cam, int row, int col, double (&d)[3]) {
  const double x = ((double)col - cam.cx_pix) / cam.focal_x;
  const double y = ((double)row - cam.cy_pix) / cam.focal_y;
  GEO_UNROLL
  for (int a = 0; a < 3; ++a) d[a] = (x * cam.M[a] + y * cam.M[3 + a]) + cam.M[6 + a];
}

// [near, far] cut to the box of voxel centres -> false for a miss (NaN too).
GEO_FN bool tsdf_ray_clip(const TsdfRayGrid& g, const TsdfRayCamera& cam, const double (&d)[3], double* z0_out, double* z1_out) {
  const int n[3] = {g.nx, g.ny, g.nz};
  double z0 = cam.near, z1 = cam.far;
  bool inside = true;
  GEO_UNROLL
  for (int a = 0; a < 3; ++a) {
    const double lo = g.origin[a] + 0.5 * g.voxel_size, hi = g.origin[a] + ((double)n[a] - 0.5) * g.voxel_size;
    if (d[a] == 0.0) {
      inside = inside && lo <= cam.c[a] && cam.c[a] <= hi;
    } else {
      double t0 = (lo - cam.c[a]) / d[a], t1 = (hi - cam.c[a]) / d[a];
      if (t0 > t1) { const double t = t0; t0 = t1; t1 = t; }
      if (t0 > z0) z0 = t0;
      if (t1 < z1) z1 = t1;
    }
  }
  *z0_out = z0; *z1_out = z1;
  return inside && z0 <= z1;
}

// Samples on [z0, z1]: floor((z1 - z0) / step) + 1, capped on the double (a NaN quotient takes the cap).
GEO_FN int tsdf_ray_samples(double z0, double z1, double step) {
  const double q = floor((z1 - z0) / step);
  return q < (double)(TSDF_RAY_MAX_SAMPLES - 1) ? (int)q + 1 : TSDF_RAY_MAX_SAMPLES;
}

GEO_FN double tsdf_ray_depth(double z0, int k, double step) { return z0 + (double)k * step; }

// The cell of the point at depth z and the position inside it: i in [0, n - 2] and f in [0, 1], clamped on the doubles.
GEO_FN void tsdf_ray_cell(const TsdfRayGrid& g, const TsdfRayCamera& cam, const double (&d)[3], double z, int (&cell)[3], double (&f)[3]) {
  const int n[3] = {g.nx, g.ny, g.nz};
  GEO_UNROLL
  for (int a = 0; a < 3; ++a) {
    const double p = cam.c[a] + z * d[a];
    const double q = (p - g.origin[a]) * g.inv_voxel - 0.5;
    double i = floor(q);
    if (!(i >= 0.0)) i = 0.0;                                             // NaN too
    if (i > (double)(n[a] - 2)) i = (double)(n[a] - 2);
    double r = q - i;
    if (!(r >= 0.0)) r = 0.0;
    if (r > 1.0) r = 1.0;
    cell[a] = (int)i;
    f[a] = r;
  }
}

// The eight corners of a cell (in range: tsdf_ray_cell clamped it) from one plane of the volume.
GEO_FN void tsdf_ray_corners(const TsdfRayGrid& g, const float* __restrict__ plane, const int (&cell)[3], float (&v)[8]) {
  const long long row = g.nx, slab = (long long)g.nx * g.ny;
  const long long base = ((long long)cell[2] * g.ny + cell[1]) * g.nx + cell[0];
  GEO_UNROLL
  for (int k = 0; k < 8; ++k) v[k] = plane[base + (k & 1) + ((k >> 1) & 1) * row + ((k >> 2) & 1) * slab];
}

// Extraction's rule for a used cell.
GEO_FN bool tsdf_ray_valid(const float (&w)[8]) {
  bool ok = true;
  GEO_UNROLL
  for (int k = 0; k < 8; ++k) ok = ok && w[k] > 0.f;
  return ok;
}

GEO_FN double tsdf_trilinear(const float (&v)[8], const double (&f)[3]) {
  const double x00 = tsdf_lerp(v[0], v[1], f[0]), x10 = tsdf_lerp(v[2], v[3], f[0]);
  const double x01 = tsdf_lerp(v[4], v[5], f[0]), x11 = tsdf_lerp(v[6], v[7], f[0]);
  const double y0 = tsdf_lerp(x00, x10, f[1]), y1 = tsdf_lerp(x01, x11, f[1]);
  return tsdf_lerp(y0, y1, f[2]);
}

// The gradient of the trilinear value in index units.
GEO_FN void tsdf_trilinear_gradient(const float (&v)[8], const double (&f)[3], double (&grad)[3]) {
  const double v0 = v[0], v1 = v[1], v2 = v[2], v3 = v[3], v4 = v[4], v5 = v[5], v6 = v[6], v7 = v[7];
  const double x00 = tsdf_lerp(v0, v1, f[0]), x10 = tsdf_lerp(v2, v3, f[0]);
  const double x01 = tsdf_lerp(v4, v5, f[0]), x11 = tsdf_lerp(v6, v7, f[0]);
  const double y0 = tsdf_lerp(x00, x10, f[1]), y1 = tsdf_lerp(x01, x11, f[1]);
  grad[2] = y1 - y0;
  grad[1] = tsdf_lerp(x10 - x00, x11 - x01, f[2]);
  grad[0] = tsdf_lerp(tsdf_lerp(v1 - v0, v3 - v2, f[1]), tsdf_lerp(v5 - v4, v7 - v6, f[1]), f[2]);
}

// Sample k of a ray -> valid?, and its value when it is.
GEO_FN bool tsdf_ray_sample(const TsdfRayGrid& g, const float* __restrict__ tsdf, const float* __restrict__ weight, const int (&cell)[3],
                            const double (&f)[3], double* value, TsdfRayCounters* n) {
  float w[8], v[8];
  tsdf_ray_corners(g, weight, cell, w);
  tsdf_ray_corners(g, tsdf, cell, v);
  if (n) ++n->samples;
  *value = tsdf_trilinear(v, f);
  return tsdf_ray_valid(w);
}

// How many lattice steps a sample at (cell, f) may advance and stay in its cell's brick, out of `left`: from where the ray leaves
// the brick's slab along each axis (inv_dq: lattice steps per cell), less one. A proposal only: the caller tests the far end.
GEO_FN int tsdf_ray_jump(const int (&cell)[3], const double (&f)[3], const double (&inv_dq)[3], int left) {
  double t = (double)left;
  GEO_UNROLL
  for (int a = 0; a < 3; ++a) {
    const int lo = cell[a] & ~(TSDF_SKIP_BRICK - 1);
    const double q = (double)cell[a] + f[a];
    if (inv_dq[a] > 0.0) {
      const double e = ((double)(lo + TSDF_SKIP_BRICK) - q) * inv_dq[a];
      if (e < t) t = e;
    } else if (inv_dq[a] < 0.0) {
      const double e = ((double)lo - q) * inv_dq[a];
      if (e < t) t = e;
    }
  }
  return t >= 2.0 ? (int)t - 1 : 0;                                        // t <= left <= 2^20; NaN gives 0
}

// The march. -> the hit: the smallest k >= 1 whose sample is valid with a value < 0 and whose predecessor is valid with a value
// >= 0 (*vp, *vc: the two values), or 0 for none. SKIP: samples whose cell lies in a brick with a zero byte are not evaluated
// -- no corner of such a cell is inside, so its value is not below 0 -- and runs of them in one brick are jumped over; the
// predecessor of a negative sample is evaluated on demand. The same hit and the same two values either way.
template <bool SKIP>
GEO_FN int tsdf_ray_march(const TsdfRayGrid& g, const TsdfRayCamera& cam, const double (&d)[3], double z0, int K,
                          const float* __restrict__ tsdf, const float* __restrict__ weight, const unsigned char* __restrict__ skip,
                          double* vp, double* vc, TsdfRayCounters* n) {
  int cell[3];
  double f[3], value;
  if (!SKIP) {
    bool before = false;                                                   // sample k - 1 is valid with a value >= 0
    double prev = 0.0;
    for (int k = 0; k < K; ++k) {
      tsdf_ray_cell(g, cam, d, tsdf_ray_depth(z0, k, cam.step), cell, f);
      const bool valid = tsdf_ray_sample(g, tsdf, weight, cell, f, &value, n);
      if (valid && value < 0.0 && before) { *vp = prev; *vc = value; return k; }
      before = valid && value >= 0.0;
      prev = value;
    }
    return 0;
  }
  double inv_dq[3];                                                        // lattice steps per cell along each axis
  GEO_UNROLL
  for (int a = 0; a < 3; ++a) {
    const double dq = cam.step * d[a] * g.inv_voxel;
    inv_dq[a] = dq != 0.0 ? 1.0 / dq : 0.0;
  }
  int known = -1;                                                          // the sample that `before` and `prev` speak of
  long long run = 0;                                                       // counted only: samples passed since the last evaluation
  bool before = false;
  double prev = 0.0;
  int k = 0;
  while (k < K) {
    tsdf_ray_cell(g, cam, d, tsdf_ray_depth(z0, k, cam.step), cell, f);
    const int b[3] = {cell[0] / TSDF_SKIP_BRICK, cell[1] / TSDF_SKIP_BRICK, cell[2] / TSDF_SKIP_BRICK};
    const bool in_table = b[0] < g.bx && b[1] < g.by && b[2] < g.bz;       // cell >= 0: the clamp
    if (in_table && skip[((long long)b[2] * g.by + b[1]) * g.bx + b[0]] == 0) {
      const int j = tsdf_ray_jump(cell, f, inv_dq, K - 1 - k);
      int step_k = 1;
      if (j >= 1) {                                                        // accepted only if sample k + j is in the same brick:
        int far_cell[3];                                                   // a cell coordinate is monotone in k
        double far_f[3];
        tsdf_ray_cell(g, cam, d, tsdf_ray_depth(z0, k + j, cam.step), far_cell, far_f);
        if (far_cell[0] / TSDF_SKIP_BRICK == b[0] && far_cell[1] / TSDF_SKIP_BRICK == b[1] && far_cell[2] / TSDF_SKIP_BRICK == b[2]) {
          step_k = j + 1;
          if (n) { ++n->jumps; if (j > n->longest) n->longest = j; }
        }
      }
      k += step_k;
      if (n) { run += step_k; if (run > n->longest_run) n->longest_run = run; }
      continue;
    }
    run = 0;
    const bool valid = tsdf_ray_sample(g, tsdf, weight, cell, f, &value, n);
    if (valid && value < 0.0 && k >= 1) {
      if (known != k - 1) {
        int pc[3];
        double pf[3];
        tsdf_ray_cell(g, cam, d, tsdf_ray_depth(z0, k - 1, cam.step), pc, pf);
        const bool pvalid = tsdf_ray_sample(g, tsdf, weight, pc, pf, &prev, n);
        before = pvalid && prev >= 0.0;
      }
      if (before) { *vp = prev; *vc = value; return k; }
    }
    known = k;
    before = valid && value >= 0.0;
    prev = value;
    ++k;
  }
  return 0;
}

// Depth, normal and colour of the hit between samples k - 1 and k with the values vp >= 0 > vc. Both ends are valid samples.
template <bool COLORS, bool NORMALS>
GEO_FN void tsdf_ray_shade(const TsdfRayGrid& g, const TsdfRayCamera& cam, const double (&d)[3], double z0, int k, double vp, double vc,
                           const float* __restrict__ tsdf, const float* __restrict__ rgb, float* depth, float (&normal)[3],
                           float (&colour)[3]) {
  const double zp = tsdf_ray_depth(z0, k - 1, cam.step), zc = tsdf_ray_depth(z0, k, cam.step);
  const double w = vp / (vp - vc);
  *depth = (float)(zp + w * (zc - zp));
  if (!COLORS && !NORMALS) return;
  int cp[3], cc[3];
  double fp[3], fc[3];
  tsdf_ray_cell(g, cam, d, zp, cp, fp);
  tsdf_ray_cell(g, cam, d, zc, cc, fc);
  float a[8], b[8];
  if (NORMALS) {
    double gp[3], gc[3], gr[3];
    tsdf_ray_corners(g, tsdf, cp, a);
    tsdf_ray_corners(g, tsdf, cc, b);
    tsdf_trilinear_gradient(a, fp, gp);
    tsdf_trilinear_gradient(b, fc, gc);
    GEO_UNROLL
    for (int i = 0; i < 3; ++i) gr[i] = gp[i] + w * (gc[i] - gp[i]);
    const double len = sqrt((gr[0] * gr[0] + gr[1] * gr[1]) + gr[2] * gr[2]);
    GEO_UNROLL
    for (int i = 0; i < 3; ++i) normal[i] = len > 0.0 ? (float)(gr[i] / len) : 0.f;
  }
  if (COLORS) {
    const long long nvox = (long long)g.nx * g.ny * g.nz;
    GEO_UNROLL
    for (int c = 0; c < 3; ++c) {
      tsdf_ray_corners(g, rgb + c * nvox, cp, a);
      tsdf_ray_corners(g, rgb + c * nvox, cc, b);
      const double p = tsdf_trilinear(a, fp), q = tsdf_trilinear(b, fc);
      colour[c] = (float)(p + w * (q - p));
    }
  }
}

// One pixel, start to end: zeros for a ray without a hit. skip is read only with SKIP.
template <bool COLORS, bool NORMALS, bool SKIP>
GEO_FN void tsdf_ray_pixel(const TsdfRayGrid& g, const TsdfRayCamera& cam, int row, int col, const float* __restrict__ tsdf,
                           const float* __restrict__ weight, const float* __restrict__ rgb, const unsigned char* __restrict__ skip,
                           float* depth, float (&normal)[3], float (&colour)[3], TsdfRayCounters* n) {
  *depth = 0.f;
  GEO_UNROLL
  for (int i = 0; i < 3; ++i) normal[i] = colour[i] = 0.f;
  double d[3], z0, z1, vp = 0.0, vc = 0.0;
  tsdf_ray_direction(cam, row, col, d);
  if (!tsdf_ray_clip(g, cam, d, &z0, &z1)) return;
  const int K = tsdf_ray_samples(z0, z1, cam.step);
  const int k = tsdf_ray_march<SKIP>(g, cam, d, z0, K, tsdf, weight, skip, &vp, &vc, n);
  if (k >= 1) tsdf_ray_shade<COLORS, NORMALS>(g, cam, d, z0, k, vp, vc, tsdf, rgb, depth, normal, colour);
}

}  // namespace sfgs
