// geo_unproject.h -- depth pixel -> world point, the float64 sequence of the reference's depth_to_point_cloud
// (evaluate_gs_geometry.py:173-204) written ONCE: geometry.hip scatters the point into a height grid, pointcloud.hip stores it,
// ortho.hip scatters its height and colour into the same grid (geo_cell: the cell rule, also written once).
// tests/geometry_np.unproject states the same sequence in numpy; both files are held to it bit for bit.
#pragma once
#include <math.h>

// GEO_FN: a device function under hipcc; a plain inline one under g++, where tests/host_check builds tsdf_math.h (and with it
// this file) for the CPU suite.
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define GEO_FN __device__ __forceinline__
#define GEO_UNROLL _Pragma("unroll")
#else
#define GEO_FN static inline
#define GEO_UNROLL
#endif

namespace sfgs {

struct GeoCamera {
  double M[9], c[3], origin[3];   // world = cam @ M + c, then + origin as a rounding step of its own
  double cx_pix, cy_pix, focal_x, focal_y;
};

// A pixel is used when depth > 0, the depth is finite (NaN fails both comparisons, +inf the second) and the mask byte,
// if there is a mask, is non-zero. p < H * W is the caller's to check.
GEO_FN bool geo_pixel_used(const float* __restrict__ depth, const unsigned char* __restrict__ mask, long long p, float* d) {
  *d = depth[p];
  return *d > 0.f && *d < INFINITY && (!mask || mask[p] != 0);
}

// (east, north, up) of pixel (row, col) at depth d. Products and sums as written, nothing contracted (-ffp-contract=off).
GEO_FN void geo_unproject(const GeoCamera& v, int row, int col, float d, double (&w)[3]) {
  const double z = (double)d;
  const double x = ((double)col - v.cx_pix) * z / v.focal_x;
  const double y = ((double)row - v.cy_pix) * z / v.focal_y;
  GEO_UNROLL
  for (int j = 0; j < 3; ++j) {
    double t = x * v.M[j] + y * v.M[3 + j];
    t = t + z * v.M[6 + j];
    t = t + v.c[j];
    w[j] = t + v.origin[j];
  }
}

// World point -> (u, v, z) in view v: pixel coordinates (columns, rows) and the depth along the camera's forward axis, the
// inverse of geo_unproject for an orthonormal M (cam = (w - c) @ M^T). v.origin is not used: consistency.hip, the one caller,
// keeps it at zero. z is not tested here; with z == 0 u and v are infinite or NaN, and the caller rejects z <= 0 first.
// tests/consistency_np.project states the same sequence in numpy.
GEO_FN void geo_project(const GeoCamera& v, const double (&w)[3], double* u, double* vv, double* z) {
  const double q0 = w[0] - v.c[0], q1 = w[1] - v.c[1], q2 = w[2] - v.c[2];
  double cam[3];
  GEO_UNROLL
  for (int a = 0; a < 3; ++a) {
    double t = q0 * v.M[3 * a] + q1 * v.M[3 * a + 1];
    cam[a] = t + q2 * v.M[3 * a + 2];
  }
  *z = cam[2];
  *u = cam[0] * v.focal_x / cam[2] + v.cx_pix;
  *vv = cam[1] * v.focal_y / cam[2] + v.cy_pix;
}

// The grid cell of a world point: geometry.hip's height grid and ortho.hip's colour grid are held to each other cell for cell.
// (int) truncates toward zero: (-1, 0) lands in cell 0, as numpy's astype(int) does. NaN fails every comparison. The open
// interval is tested on the float64 first (a value beyond int's range is never converted), the integer range after it.
GEO_FN bool geo_cell(double east, double north, double xoff, double yoff_top, double res, int xsize, int ysize,
                     int* gx_out, int* gy_out) {
  const double qx = (east - xoff) / res, qy = (yoff_top - north) / res;
  if (qx > -1.0 && qx < (double)xsize && qy > -1.0 && qy < (double)ysize) {
    const int gx = (int)qx, gy = (int)qy;
    if (gx >= 0 && gx < xsize && gy >= 0 && gy < ysize) {
      *gx_out = gx; *gy_out = gy;
      return true;
    }
  }
  return false;
}

}  // namespace sfgs
