// mesh_query_math.h -- what the mesh query kernels (mesh_query.hip) decide per element, written once for the device and for the
// host build that tests/host_check/mesh_query_check.cpp drives sequentially: the cell of a coordinate, the cells of a face, the
// closest point of a triangle, the ring search's bounds, and for the sampler the area of a face, the integer mixer and the
// position of a sample. Float64, one rounded operation at a time in the order written (build with -ffp-contract=off); nothing
// here touches memory but the words it is handed.
#pragma once
#include "mesh_math.h"

namespace sfgs {

constexpr long long MQ_MAX_GRID_CELLS = 1ll << 28;    // nx ny nz of a face grid
constexpr long long MQ_MAX_CELLS_DEFAULT = 4096;      // a face whose cell range holds more cells goes to the large list
constexpr long long MQ_MAX_CELLS_LIMIT = 1ll << 30;   // the largest max_cells: above any grid, so every face is scattered
constexpr double MQ_MARGIN = 1.0 - 1.0 / 1048576.0;   // 1 - 2^-20, exact
constexpr double MQ_CELL_LIMIT = 1073741824.0;        // 2^30: a query's cell index is clamped to +-this, beyond every grid
constexpr long long MQ_MAX_SAMPLES_PER_FACE = 1ll << 20;
// status bits of a grid / a query / a sampling beside mesh_math.h's (MESH_ST_FIND_BOUND: the segment sort's trip bound;
// MESH_ST_BAD_INDEX: a table entry out of range): the pair capacity was too small; more than 2^31 - 1 pairs; a face with a
// non-finite area or more than 2^20 samples
enum { MQ_ST_CAPACITY = 32, MQ_ST_PAIRS = 64, MQ_ST_BAD_FACE = 128 };

struct MqGrid {
  double origin[3], cell;
  int dims[3];
};

MESH_HD bool mq_finite(double x) { return x - x == 0.0; }

// THE cell function, for the vertices of a face and for a query point alike: floor((x - origin) / cell). It is monotone in x
// (a rounded difference, a rounded quotient by a positive number and floor all are), which is what the ring search's proof
// rests on. The result is an integer-valued double, or not finite when x is not.
MESH_HD double mq_cell(double x, double origin, double cell) { return floor((x - origin) / cell); }

// a cell index clamped into 0 ... dim - 1 (a face's range), and into -2^30 ... 2^30 (a query's own cell: the grid lies strictly
// inside, so a clamped query only looks nearer to the grid than it is)
MESH_HD int mq_clamp_cell(double c, int dim) { return c < 0.0 ? 0 : (c > (double)(dim - 1) ? dim - 1 : (int)c); }
MESH_HD int mq_query_cell(double c) { return c < -MQ_CELL_LIMIT ? (int)-MQ_CELL_LIMIT : (c > MQ_CELL_LIMIT ? (int)MQ_CELL_LIMIT : (int)c); }

// The cell range of the face (a, b, c): per axis the cells of the smallest and the largest coordinate, clamped into the grid.
// false when a coordinate is not finite (the face is left out). *cells = the number of cells in the range.
MESH_HD bool mq_face_range(const MqGrid& g, const float* a, const float* b, const float* c, int* lo, int* hi, long long* cells) {
  long long prod = 1;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float mn = a[k] < b[k] ? (a[k] < c[k] ? a[k] : c[k]) : (b[k] < c[k] ? b[k] : c[k]);
    const float mx = a[k] > b[k] ? (a[k] > c[k] ? a[k] : c[k]) : (b[k] > c[k] ? b[k] : c[k]);
    ok = ok && mq_finite((double)a[k]) && mq_finite((double)b[k]) && mq_finite((double)c[k]);
    lo[k] = ok ? mq_clamp_cell(mq_cell((double)mn, g.origin[k], g.cell), g.dims[k]) : 0;
    hi[k] = ok ? mq_clamp_cell(mq_cell((double)mx, g.origin[k], g.cell), g.dims[k]) : 0;
    prod *= (long long)(hi[k] - lo[k] + 1);
  }
  *cells = prod;
  return ok;
}

MESH_HD double mq_dot(const double* u, const double* v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

// The closest point of the closed triangle (a, b, c) to p, and its squared distance. The regions are decided in this order:
// vertex a, vertex b, edge ab, vertex c, edge ac, edge bc, interior; each value is formed by the one expression written here.
// A quotient whose denominator is not positive (a face without area) is taken as 0, so a degenerate face still answers with
// one of its own points. Returns d2 = |p - q|^2; q goes to `out`.
MESH_HD double mq_closest(const double* p, const float* fa, const float* fb, const float* fc, double* out) {
  double a[3], ab[3], ac[3], ap[3], bp[3], cp[3], bc[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    a[k] = (double)fa[k];
    ab[k] = (double)fb[k] - a[k];
    ac[k] = (double)fc[k] - a[k];
    bc[k] = (double)fc[k] - (double)fb[k];
    ap[k] = p[k] - a[k];
    bp[k] = p[k] - (double)fb[k];
    cp[k] = p[k] - (double)fc[k];
  }
  const double d1 = mq_dot(ab, ap), d2 = mq_dot(ac, ap), d3 = mq_dot(ab, bp), d4 = mq_dot(ac, bp), d5 = mq_dot(ab, cp), d6 = mq_dot(ac, cp);
  const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  const double e43 = d4 - d3, e56 = d5 - d6;
  double q[3];
  if (d1 <= 0.0 && d2 <= 0.0) {
    for (int k = 0; k < 3; ++k) q[k] = a[k];
  } else if (d3 >= 0.0 && d4 <= d3) {
    for (int k = 0; k < 3; ++k) q[k] = (double)fb[k];
  } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
    const double den = d1 - d3, v = den > 0.0 ? d1 / den : 0.0;
    for (int k = 0; k < 3; ++k) q[k] = a[k] + v * ab[k];
  } else if (d6 >= 0.0 && d5 <= d6) {
    for (int k = 0; k < 3; ++k) q[k] = (double)fc[k];
  } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
    const double den = d2 - d6, w = den > 0.0 ? d2 / den : 0.0;
    for (int k = 0; k < 3; ++k) q[k] = a[k] + w * ac[k];
  } else if (va <= 0.0 && e43 >= 0.0 && e56 >= 0.0) {
    const double den = e43 + e56, w = den > 0.0 ? e43 / den : 0.0;
    for (int k = 0; k < 3; ++k) q[k] = (double)fb[k] + w * bc[k];
  } else {
    const double s = (va + vb) + vc, v = s > 0.0 ? vb / s : 0.0, w = s > 0.0 ? vc / s : 0.0;
    for (int k = 0; k < 3; ++k) q[k] = (a[k] + v * ab[k]) + w * ac[k];
  }
  double d[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { d[k] = p[k] - q[k]; out[k] = q[k]; }
  return mq_dot(d, d);
}

// (d2, face) against the best so far: a d2 that is not finite never wins, equal d2 goes to the smaller face index
MESH_HD bool mq_better(double d2, int32_t face, double best_d2, int32_t best_face) {
  return mq_finite(d2) && (d2 < best_d2 || (d2 == best_d2 && (best_face < 0 || face < best_face)));
}

// The ring search. After every cell within Chebyshev distance r of the query's own cell has been visited, r at least the first
// ring that meets the grid, a face registered in none of them has, on some axis, a coordinate whose cell index differs from the
// query's by more than r (its range was clamped only toward visited cells); mq_cell is monotone and shared, so that coordinate
// lies at least r cell (1 - 2^-40) from the query's. The search stops once best_d2 < (r cell)^2 (1 - 2^-20) -- no face left can
// win or tie -- or once r cell (1 - 2^-20) > max_distance. Below the first ring the rule does not hold: a face outside the
// grid sits in a border cell, however near a query outside the grid it is.
MESH_HD double mq_ring_d2(int r, double cell) { const double rc = (double)r * cell; return (rc * rc) * MQ_MARGIN; }
MESH_HD bool mq_ring_beyond(int r, double cell, double max_distance) { return ((double)r * cell) * MQ_MARGIN > max_distance; }

// the first ring around cell q that meets 0 ... dim - 1 on this axis, and the last that still holds a cell of it
MESH_HD int mq_ring_first(int q, int dim) { return q < 0 ? -q : (q > dim - 1 ? q - (dim - 1) : 0); }
MESH_HD int mq_ring_last(int q, int dim) {
  const int lo = q < 0 ? -q : q, far = dim - 1 - q, hi = far < 0 ? -far : far;
  return lo > hi ? lo : hi;
}

// ---- the sampler ----------------------------------------------------------------------------------------------------------------
// the area of a face: half the norm of mesh_face_normal's cross product
MESH_HD double mq_area(const float* a, const float* b, const float* c) {
  double n[3];
  mesh_face_normal(a, b, c, n);
  return 0.5 * sqrt(mq_dot(n, n));
}

// the 32-bit mixer of (seed, face, counter): mesh_mix over a running fold of the three words, uint32 arithmetic throughout
MESH_HD uint32_t mq_mix3(uint32_t seed, uint32_t face, uint32_t counter) {
  uint32_t h = mesh_mix(seed ^ 0x9e3779b9u);
  h = mesh_mix(h ^ face * 0x7feb352du);
  h = mesh_mix(h ^ counter * 0x846ca68bu);
  return h;
}
MESH_HD double mq_unit(uint32_t h) { return ((double)h + 0.5) * MESH_FIX_INV; }    // (h + 0.5) / 2^32, exact, in (0, 1)

// samples of a face of area A at `density`: floor(e) + (u < e - floor(e)), e = A density, u from the mixer at counter all-ones.
// -1 when e is not finite or the count exceeds 2^20 (the face samples nothing and raises the status).
MESH_HD long long mq_sample_count(double area, double density, uint32_t seed, uint32_t face) {
  const double e = area * density, fl = floor(e);
  if (!mq_finite(e) || fl > (double)MQ_MAX_SAMPLES_PER_FACE) return -1;
  const long long cnt = (long long)fl + (mq_unit(mq_mix3(seed, face, 0xffffffffu)) < e - fl ? 1 : 0);
  return cnt > MQ_MAX_SAMPLES_PER_FACE ? -1 : cnt;
}

// sample j of a face: (u1, u2) from the mixer at counters 2 j and 2 j + 1, reflected when u1 + u2 > 1; -> the weights
MESH_HD void mq_sample_uv(uint32_t seed, uint32_t face, uint32_t j, double* u1, double* u2) {
  double a = mq_unit(mq_mix3(seed, face, 2u * j)), b = mq_unit(mq_mix3(seed, face, 2u * j + 1u));
  if (a + b > 1.0) { a = 1.0 - a; b = 1.0 - b; }
  *u1 = a; *u2 = b;
}
// an attribute (a position, a colour) at the weights: float32((a + u1 (b - a)) + u2 (c - a)) in float64
MESH_HD float mq_sample_attr(float a, float b, float c, double u1, double u2) {
  const double da = (double)a;
  return (float)((da + u1 * ((double)b - da)) + u2 * ((double)c - da));
}

}  // namespace sfgs
