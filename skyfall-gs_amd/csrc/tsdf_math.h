// tsdf_math.h -- the per-voxel update of TSDF fusion and the per-cell marching-tetrahedra triangulation, written ONCE: tsdf.hip
// runs them on the device, tests/host_check/tsdf_check.cpp builds them with g++ for the CPU suite (GEO_FN: geo_unproject.h), and
// tests/tsdf_np.py states both in numpy; the three are held to each other byte for byte. include/sfgs.h gives the sequences in
// words. Nothing is contracted (-ffp-contract=off on both compilers): products, sums and quotients in the order written.
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

}  // namespace sfgs
