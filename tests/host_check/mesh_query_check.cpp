// The host build of csrc/mesh_query_math.h: the functions csrc/mesh_query.hip runs per face, query and sample, driven by plain
// sequential loops (tests/mesh_query_hostcheck.py binds this file with ctypes). Build: g++ -O2 -ffp-contract=off.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <vector>

#include "../../skyfall-gs_amd/csrc/mesh_query_math.h"

using namespace sfgs;

namespace {

MqGrid grid_of(const double* origin, double cell, const int* dims) {
  MqGrid g;
  for (int k = 0; k < 3; ++k) { g.origin[k] = origin[k]; g.dims[k] = dims[k]; }
  g.cell = cell;
  return g;
}

bool load_face(const float* V, const int32_t* F, long long t, long long m, const float** a, const float** b, const float** c) {
  const int32_t ia = F[3 * t], ib = F[3 * t + 1], ic = F[3 * t + 2];
  if (!(mesh_index_ok(ia, m) && mesh_index_ok(ib, m) && mesh_index_ok(ic, m))) return false;
  *a = V + 3ll * ia; *b = V + 3ll * ib; *c = V + 3ll * ic;
  return true;
}

// 0 left out, 1 scattered, 2 large
int classify(const MqGrid& g, const float* V, const int32_t* F, long long t, long long m, long long max_cells, int* lo, int* hi) {
  const float *a, *b, *c;
  long long cells;
  if (!load_face(V, F, t, m, &a, &b, &c) || !mq_face_range(g, a, b, c, lo, hi, &cells)) return 0;
  return cells > max_cells ? 2 : 1;
}

struct Best { double d2, q[3]; int32_t face; };

void test_face(const float* V, const int32_t* F, long long m, long long n, const double* p, long long t, Best* best) {
  const float *a, *b, *c;
  if (t < 0 || t >= n || !load_face(V, F, t, m, &a, &b, &c)) return;
  double q[3];
  const double d2 = mq_closest(p, a, b, c, q);
  if (mq_better(d2, (int32_t)t, best->d2, best->face)) { best->d2 = d2; best->face = (int32_t)t; memcpy(best->q, q, sizeof q); }
}

}  // namespace

extern "C" double mqc_cell(double x, double origin, double cell) { return mq_cell(x, origin, cell); }

extern "C" double mqc_area(const float* tri) { return mq_area(tri, tri + 3, tri + 6); }

extern "C" uint32_t mqc_mix3(uint32_t seed, uint32_t face, uint32_t counter) { return mq_mix3(seed, face, counter); }

// one point against faces 0 ... n - 1 (a face with an index out of range: NaN) -> d2 [n], q [n][3]
extern "C" void mqc_closest_faces(const double* p, const float* V, const int32_t* F, long long m, long long n, double* d2, double* q) {
  for (long long t = 0; t < n; ++t) {
    const float *a, *b, *c;
    if (!load_face(V, F, t, m, &a, &b, &c)) { d2[t] = q[3 * t] = q[3 * t + 1] = q[3 * t + 2] = std::numeric_limits<double>::quiet_NaN(); continue; }
    d2[t] = mq_closest(p, a, b, c, q + 3 * t);
  }
}

// the CSR table, sequentially: cell_start [cells + 1], pairs [capacity] (nothing at or beyond it), large [n] ascending,
// state [4] = pairs, large, status, left out. pairs == NULL: counts only.
extern "C" void mqc_grid(const float* V, const int32_t* F, long long m, long long n, const double* origin, double cell, const int* dims,
                         long long max_cells, int32_t* cell_start, int32_t* pairs, long long capacity, int32_t* large, long long* state) {
  const MqGrid g = grid_of(origin, cell, dims);
  const long long cells = (long long)dims[0] * dims[1] * dims[2];
  std::vector<long long> count(cells + 1, 0);
  memset(state, 0, 4 * sizeof(long long));
  int lo[3], hi[3];
  for (int pass = 0; pass < 2; ++pass) {
    for (long long t = 0; t < n; ++t) {
      const int kind = classify(g, V, F, t, m, max_cells, lo, hi);
      if (pass == 0 && kind == 0) ++state[3];
      if (pass == 0 && kind == 2) large[state[1]++] = (int32_t)t;
      if (kind != 1) continue;
      for (int z = lo[2]; z <= hi[2]; ++z)
        for (int y = lo[1]; y <= hi[1]; ++y)
          for (int x = lo[0]; x <= hi[0]; ++x) {
            const long long c = ((long long)z * dims[1] + y) * dims[0] + x;
            if (pass == 0) { ++count[c]; ++state[0]; }
            else { const long long pos = count[c]++; if (pos < capacity) pairs[pos] = (int32_t)t; }      // faces ascend: so do the runs
          }
    }
    if (pass == 0) {
      long long run = 0;
      for (long long c = 0; c <= cells; ++c) { const long long k = count[c]; count[c] = run; cell_start[c] = (int32_t)run; run += k; }
      if (state[0] > capacity && pairs) state[2] |= MQ_ST_CAPACITY;
      if (!pairs) return;
    }
  }
}

// the search of mq_closest_kernel for k float64 points, sequentially; rings (or NULL): the rings each query visited
extern "C" void mqc_search(const float* V, const int32_t* F, long long m, long long n, const double* origin, double cell, const int* dims,
                           const int32_t* cell_start, const int32_t* pairs, long long npairs, const int32_t* large, long long nlarge,
                           const double* points, long long k, double max_distance, double* sqdist, int32_t* face, float* closest,
                           long long* counts, int32_t* rings) {
  const MqGrid g = grid_of(origin, cell, dims);
  const double max_d2 = max_distance * max_distance;
  counts[0] = counts[1] = 0;
  for (long long i = 0; i < k; ++i) {
    const double* p = points + 3 * i;
    Best best;
    best.d2 = std::numeric_limits<double>::infinity(); best.face = -1; best.q[0] = best.q[1] = best.q[2] = 0.0;
    int visited = 0;
    if (mq_finite(p[0]) && mq_finite(p[1]) && mq_finite(p[2])) {
      for (long long j = 0; j < nlarge; ++j) test_face(V, F, m, n, p, large[j], &best);
      long long q[3];
      int r0 = 0, r1 = 0;
      for (int a = 0; a < 3; ++a) {
        const int qa = mq_query_cell(mq_cell(p[a], g.origin[a], g.cell));
        q[a] = qa; r0 = std::max(r0, mq_ring_first(qa, dims[a])); r1 = std::max(r1, mq_ring_last(qa, dims[a]));
      }
      if (npairs > 0) {
        for (long long r = r0; r <= r1; ++r) {
          ++visited;
          long long c0[3], c1[3];
          for (int a = 0; a < 3; ++a) { c0[a] = std::max(q[a] - r, 0ll); c1[a] = std::min(q[a] + r, (long long)dims[a] - 1); }
          for (long long z = c0[2]; z <= c1[2]; ++z)
            for (long long y = c0[1]; y <= c1[1]; ++y) {
              const bool shell = z - q[2] == r || q[2] - z == r || y - q[1] == r || q[1] - y == r;
              for (long long x = c0[0]; x <= c1[0]; ++x) {
                if (!shell && x != q[0] - r && x != q[0] + r) continue;
                const long long c = (z * dims[1] + y) * dims[0] + x;
                for (long long j = cell_start[c]; j < cell_start[c + 1] && j < npairs; ++j) test_face(V, F, m, n, p, pairs[j], &best);
              }
            }
          if (best.d2 < mq_ring_d2((int)r, cell) || mq_ring_beyond((int)r, cell, max_distance)) break;
        }
      }
    }
    if (best.face >= 0 && best.d2 > max_d2) best.face = -1;
    if (best.face < 0) { best.d2 = std::numeric_limits<double>::infinity(); best.q[0] = best.q[1] = best.q[2] = 0.0; }
    sqdist[i] = best.d2; face[i] = best.face;
    if (closest) for (int a = 0; a < 3; ++a) closest[3 * i + a] = (float)best.q[a];
    ++counts[best.face >= 0 ? 0 : 1];
    if (rings) rings[i] = visited;
  }
}

// the sampler, sequentially; points == NULL: counts only. state [4] = samples found, 0, status, 0
extern "C" void mqc_sample(const float* V, const float* C, const int32_t* F, long long m, long long n, double density, uint32_t seed,
                           long long capacity, float* points, int32_t* face, float* colors, long long* state) {
  memset(state, 0, 4 * sizeof(long long));
  for (long long t = 0; t < n; ++t) {
    const float *a, *b, *c;
    if (!load_face(V, F, t, m, &a, &b, &c)) { state[2] |= MESH_ST_BAD_INDEX; continue; }
    const long long cnt = mq_sample_count(mq_area(a, b, c), density, seed, (uint32_t)t);
    if (cnt < 0) { state[2] |= MQ_ST_BAD_FACE; continue; }
    for (long long j = 0; j < cnt; ++j) {
      const long long row = state[0]++;
      if (!points || row >= capacity) continue;
      double u1, u2;
      mq_sample_uv(seed, (uint32_t)t, (uint32_t)j, &u1, &u2);
      face[row] = (int32_t)t;
      for (int k = 0; k < 3; ++k) {
        points[3 * row + k] = mq_sample_attr(a[k], b[k], c[k], u1, u2);
        if (colors) colors[3 * row + k] = mq_sample_attr(C[3ll * F[3 * t] + k], C[3ll * F[3 * t + 1] + k], C[3ll * F[3 * t + 2] + k], u1, u2);
      }
    }
  }
}
