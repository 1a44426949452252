// mesh_math.h -- what the mesh kernels (mesh.hip) decide per element, written once for the device and for the host build that
// tests/host_check/mesh_check.cpp drives sequentially: the vertex key and its hash, the table's size, the face rules (integers
// only), and for decimation and vertex normals (tests/host_check/mesh_simplify_check.cpp) the cell of a vertex, the fixed-point
// means and the face normal in float64. Nothing here touches memory but the words it is handed.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MESH_HD __host__ __device__ __forceinline__
#else
#define MESH_HD inline
#endif

namespace sfgs {

constexpr uint32_t MESH_EMPTY = 0xffffffffu;          // a hash slot that holds no soup vertex index (3 n <= 3 * 2^29 < this)
constexpr long long MESH_MAX_TRIANGLES = 1ll << 29;   // 3 n fits int32
constexpr long long MESH_MAX_VERTICES = 0x7fffffffll;
constexpr int MESH_CAS_RETRIES = 1 << 16;             // hooks that may fail in a row on one edge before the kernel gives up
// status bits (state word 2 of a mesh, word 1 of a component result): 0 = everything ran to its end
// (MESH_ST_FIND_BOUND is also what the adjacency's segment sort raises at its trip bound; MESH_ST_BAD_VERTEX: a vertex whose cell is
// not finite or leaves int32 was met by the decimation and joined no cluster)
enum { MESH_ST_PROBE_BOUND = 1, MESH_ST_FIND_BOUND = 2, MESH_ST_CAS_BOUND = 4, MESH_ST_BAD_INDEX = 8, MESH_ST_BAD_VERTEX = 16 };

// A vertex key is the three 32-bit words of its position, compared as bit patterns: -0.0 != +0.0, NaNs equal when their bits are.
struct MeshKey { uint32_t w[3]; };

MESH_HD MeshKey mesh_key(const uint32_t* soup_words, long long q) {
  MeshKey k;
  k.w[0] = soup_words[3 * q]; k.w[1] = soup_words[3 * q + 1]; k.w[2] = soup_words[3 * q + 2];
  return k;
}
MESH_HD bool mesh_key_equal(const MeshKey& a, const MeshKey& b) { return a.w[0] == b.w[0] && a.w[1] == b.w[1] && a.w[2] == b.w[2]; }

// murmur3's 32-bit finaliser over a running mix of the three words
MESH_HD uint32_t mesh_mix(uint32_t h) {
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  return h;
}
MESH_HD uint32_t mesh_hash(const MeshKey& k) {
  uint32_t h = mesh_mix(k.w[0] ^ 0x9e3779b9u);
  h = mesh_mix(h ^ k.w[1] * 0x7feb352du);      // (the product binds first: the word is spread before it is folded in)
  h = mesh_mix(h ^ k.w[2] * 0x846ca68bu);
  return h;
}

// slots of the weld's table for n triangles: the power of two >= 2 * 3 n, at least 64 (load factor <= 1/2)
MESH_HD unsigned long long mesh_weld_slots(long long n) {
  unsigned long long s = 64;
  while (s < 6ull * (unsigned long long)n) s <<= 1;
  return s;
}

MESH_HD bool mesh_index_ok(int32_t v, long long m) { return v >= 0 && (long long)v < m; }
MESH_HD bool mesh_face_degenerate(int32_t a, int32_t b, int32_t c) { return a == b || b == c || a == c; }

// ---- decimation by vertex clustering and vertex normals: float64, one rounded operation at a time (build with -ffp-contract=off)
constexpr double MESH_FIX_ONE = 4294967296.0;          // 2^32: the fixed point of a position inside its cell, and of a colour
constexpr double MESH_FIX_INV = 1.0 / 4294967296.0;    // 2^-32, exact
constexpr int MESH_SORT_SHORT = 32;                    // adjacency segments up to this long are insertion-sorted, longer ones heap-sorted

// slots of a table for `keys` keys: the power of two >= 2 keys, at least 64 (mesh_weld_slots over keys / 3 rounded up)
MESH_HD unsigned long long mesh_key_slots(long long keys) { return mesh_weld_slots((keys + 2) / 3); }

// One axis of a vertex's cell: u = (x - origin) / cell, i = floor(u), f = u - i in [0, 1], p = floor(f 2^32) <= 2^32.
// false (the vertex is bad) when u is not finite or i lies outside int32; then *i and *p are 0.
MESH_HD bool mesh_cell_axis(float x, double origin, double cell, int32_t* i, uint64_t* p) {
  const double u = ((double)x - origin) / cell;
  const double fl = floor(u);
  *i = 0; *p = 0;
  if (!(u - u == 0.0) || fl < -2147483648.0 || fl > 2147483647.0) return false;       // u - u is 0 exactly when u is finite
  const double f = u - fl;
  *i = (int32_t)fl;
  *p = (uint64_t)floor(f * MESH_FIX_ONE);
  return true;
}

// the position of a cluster of c >= 2 members along one axis from its cell index and the sum of its members' p
MESH_HD float mesh_cell_resolve(int32_t i, uint64_t sum, uint32_t c, double origin, double cell) {
  const double inside = (double)(sum / c) * MESH_FIX_INV;
  return (float)(((double)i + inside) * cell + origin);
}

// a colour component as fixed point: NaN -> 0, clamped to [0, 1] in float64, floor(x 2^32) <= 2^32; and the mean back
MESH_HD uint64_t mesh_color_fix(float x) {
  double d = (double)x;
  if (d != d) d = 0.0;
  d = d < 0.0 ? 0.0 : (d > 1.0 ? 1.0 : d);
  return (uint64_t)floor(d * MESH_FIX_ONE);
}
MESH_HD float mesh_color_resolve(uint64_t sum, uint32_t c) { return (float)((double)(sum / c) * MESH_FIX_INV); }

// the three indices of a face in ascending order: the key under which faces over the same SET of vertices meet
MESH_HD void mesh_sorted_triple(int32_t a, int32_t b, int32_t c, uint32_t* out) {
  int32_t t;
  if (a > b) { t = a; a = b; b = t; }
  if (b > c) { t = b; b = c; c = t; }
  if (a > b) { t = a; a = b; b = t; }
  out[0] = (uint32_t)a; out[1] = (uint32_t)b; out[2] = (uint32_t)c;
}

// the area-weighted normal of the face (a, b, c), in float64 from the float32 positions: (b - a) x (c - a)
MESH_HD void mesh_face_normal(const float* a, const float* b, const float* c, double* n) {
  const double e1x = (double)b[0] - (double)a[0], e1y = (double)b[1] - (double)a[1], e1z = (double)b[2] - (double)a[2];
  const double e2x = (double)c[0] - (double)a[0], e2y = (double)c[1] - (double)a[1], e2z = (double)c[2] - (double)a[2];
  n[0] = e1y * e2z - e1z * e2y;
  n[1] = e1z * e2x - e1x * e2z;
  n[2] = e1x * e2y - e1y * e2x;
}

// float32(N / len) per component with len = sqrt((Nx Nx + Ny Ny) + Nz Nz) when len > 0 and finite, else (0, 0, 0)
MESH_HD void mesh_normalize(const double* N, float* out) {
  const double len = sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2]);
  if (len > 0.0 && len - len == 0.0) {
    out[0] = (float)(N[0] / len); out[1] = (float)(N[1] / len); out[2] = (float)(N[2] / len);
  } else {
    out[0] = 0.f; out[1] = 0.f; out[2] = 0.f;
  }
}

}  // namespace sfgs
