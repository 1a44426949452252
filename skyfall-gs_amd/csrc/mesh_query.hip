// mesh_query.hip -- measuring a mesh: a uniform grid over its faces (sfgs_mesh_grid_count / sfgs_mesh_grid_fill; Python:
// Mesh.face_grid), the closest face of a point (sfgs_mesh_closest; Mesh.closest) and points on the surface, uniform per area
// (sfgs_mesh_sample; Mesh.sample). include/sfgs.h states the results in words, tests/mesh_query_np.py in numpy,
// mesh_query_math.h holds every per-element function; the kernels equal the restatement byte for byte.
//   GRID. mq_count_kernel: a thread per face decides left out / scattered / large with mq_face_range and adds 1 to the count of
//     every cell of a scattered face's range (relaxed integer atomics); the pair total is summed per wave in 64 bits, a large
//     face is appended to the large list with one counter atomic per wave. The list holds n entries and a face is appended at
//     most once: it cannot overflow. An exclusive scan of the counts in the three launches of the compaction's plan (the middle
//     one is scan.h's loop) gives cell_start. mq_fill_kernel: the same decision again, the face index through atomic cursors into
//     `pairs`, never at or beyond `capacity`; then mesh.hip's vf_sort_kernel, a thread per cell, sorts each cell's run ascending,
//     so the table is the same bytes run after run. A thread's fill loop is bounded by max_cells.
//   CLOSEST. mq_closest_kernel: a thread per query (a wave per query is the variant next to MQ_WAVE_PER_QUERY). It tests every face of the large list, then the Chebyshev rings of cells
//     around the query's own cell, from the first that meets the grid, and stops by the rule next to mq_ring_d2
//     (mesh_query_math.h), at the latest after the ring that holds the grid's farthest cell. The winner is the minimum of
//     (d2, face index); each query's result is written by its own lane: no atomics on the outputs, no float atomics. The counts are
//     summed per wave. Every index is checked before its use: a cell's run against the pair capacity, a pair against n, a face's
//     three against m.
//   SAMPLE. mq_sample_count_kernel (a thread per face: its count from the area and the mixer), the same scan, mq_sample_emit_kernel
//     (a thread per face writes its rows in order, never at or beyond `capacity`; its loop is bounded by 2^20).
//   SUMMARY. mq_summary_kernel (sfgs_mesh_distance_summary; MeshDistance.summary): one launch; per-workgroup float64 partials in a
//     fixed order, integer counts, and the workgroup that draws the last ticket adds the partials in index order.
// No LDS beyond the scans' and the summary's trees, no profiler ids.
#include "sfgs_internal.h"
#include "mesh_query_math.h"
#include "scan.h"

namespace sfgs {

constexpr int MQ_THREADS = 256;
#define MQ_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
enum { MQ_STATE_STATUS = 2 };                // as a mesh's: state word 2 is the status (vf_sort_kernel raises it there)
enum { MQ_LEFT_OUT = 0, MQ_SCATTERED = 1, MQ_LARGE = 2 };

// the segment sort of mesh.hip (a thread per segment, ascending in place; insertion sort up to 32 records, heapsort beyond)
__global__ void vf_sort_kernel(const int32_t* __restrict__ offsets, long long m, long long Q, int32_t* __restrict__ records,
                               long long* __restrict__ state);

__device__ __forceinline__ void mq_raise(long long* state, unsigned bits) {
  __hip_atomic_fetch_or((unsigned long long*)&state[MQ_STATE_STATUS], (unsigned long long)bits, MQ_RLX);
}

__device__ __forceinline__ unsigned long long mq_wave_sum(unsigned long long v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
  return v;                                   // lane 0 holds the wave's sum
}

__device__ __forceinline__ bool mq_load_face(const float* __restrict__ vertices, const int32_t* __restrict__ faces, long long t,
                                             long long m, float (&a)[3], float (&b)[3], float (&c)[3]) {
  const int32_t ia = faces[3 * t], ib = faces[3 * t + 1], ic = faces[3 * t + 2];
  if (!(mesh_index_ok(ia, m) && mesh_index_ok(ib, m) && mesh_index_ok(ic, m))) return false;
  load3(vertices + 3ll * ia, a); load3(vertices + 3ll * ib, b); load3(vertices + 3ll * ic, c);
  return true;
}

__device__ __forceinline__ int mq_classify(const MqGrid& g, const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                           long long t, long long m, long long max_cells, int* lo, int* hi, long long* cells) {
  float a[3], b[3], c[3];
  *cells = 0;
  if (!mq_load_face(vertices, faces, t, m, a, b, c)) return MQ_LEFT_OUT;
  if (!mq_face_range(g, a, b, c, lo, hi, cells)) return MQ_LEFT_OUT;
  return *cells > max_cells ? MQ_LARGE : MQ_SCATTERED;
}

__device__ __forceinline__ long long mq_cell_index(const MqGrid& g, long long x, long long y, long long z) {
  return (z * g.dims[1] + y) * g.dims[0] + x;
}

// ---- the grid ----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MQ_THREADS)
mq_count_kernel(MqGrid g, const float* __restrict__ vertices, const int32_t* __restrict__ faces, long long m, long long n,
                long long max_cells, uint32_t* count, int32_t* __restrict__ large, long long* state) {
  const long long t = (long long)blockIdx.x * MQ_THREADS + threadIdx.x;
  int kind = -1, lo[3], hi[3];
  long long cells = 0;
  if (t < n) kind = mq_classify(g, vertices, faces, t, m, max_cells, lo, hi, &cells);
  if (kind == MQ_SCATTERED) {
    for (int z = lo[2]; z <= hi[2]; ++z)
      for (int y = lo[1]; y <= hi[1]; ++y)
        for (int x = lo[0]; x <= hi[0]; ++x) __hip_atomic_fetch_add(&count[mq_cell_index(g, x, y, z)], 1u, MQ_RLX);
  }
  const unsigned lane = lane_id();
  const unsigned long long pairs = mq_wave_sum(kind == MQ_SCATTERED ? (unsigned long long)cells : 0ull);
  if (lane == 0 && pairs) __hip_atomic_fetch_add((unsigned long long*)&state[0], pairs, MQ_RLX);
  const unsigned long long out = __ballot(kind == MQ_LEFT_OUT);
  if (lane == 0 && out) __hip_atomic_fetch_add((unsigned long long*)&state[3], (unsigned long long)__popcll(out), MQ_RLX);
  const unsigned long long lb = __ballot(kind == MQ_LARGE);
  if (lb) {
    unsigned long long base = 0;
    if (lane == 0) base = __hip_atomic_fetch_add((unsigned long long*)&state[1], (unsigned long long)__popcll(lb), MQ_RLX);
    base = __shfl(base, 0);
    if (kind == MQ_LARGE) {
      const unsigned long long at = base + (unsigned long long)__popcll(lb & ((1ull << lane) - 1ull));
      if (at < (unsigned long long)n) large[at] = (int32_t)t;           // always: a face is appended at most once
      else mq_raise(state, MESH_ST_PROBE_BOUND);
    }
  }
}

// the exclusive scan of N counts in the three launches of the row compaction's plan: sums per CP_CHUNK, ONE workgroup over the sums
// (scan.h), then the offsets and the cursors that start at them. offsets[N] = the total's low 31 bits; the 64-bit total in
// state word 0 (summed by the counting kernel) is what decides: beyond 2^31 - 1 it raises MQ_ST_PAIRS and the table is not valid.
__global__ void __launch_bounds__(CP_NT)
mq_chunk_sum_kernel(const uint32_t* __restrict__ count, long long N, unsigned* __restrict__ block_sum) {
  __shared__ unsigned smem[CP_NT / 64 + 1];
  const long long base = (long long)blockIdx.x * CP_CHUNK + (long long)threadIdx.x * CP_ROWS_PER_THREAD;
  unsigned c = 0;
#pragma unroll
  for (int k = 0; k < CP_ROWS_PER_THREAD; ++k) c += base + k < N ? count[base + k] : 0u;
  unsigned total;
  block_excl_scan_u32<CP_NT>(c, &total, smem);
  if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

__global__ void __launch_bounds__(SCAN_TOP_THREADS)
mq_scan_top_kernel(unsigned* __restrict__ block_sum, long long NB, int32_t* __restrict__ last, long long* state) {
  __shared__ unsigned smem[SCAN_TOP_THREADS / 64 + 1];
  const unsigned long long total = scan_sums_excl(block_sum, NB, 1, 0ull, smem);
  if (threadIdx.x == 0) {
    *last = (int32_t)(total & 0x7fffffffull);
    if (state[0] > 0x7fffffffll) mq_raise(state, MQ_ST_PAIRS);
  }
}

__global__ void __launch_bounds__(CP_NT)
mq_offsets_kernel(uint32_t* __restrict__ count_cursor, long long N, const unsigned* __restrict__ block_sum, int32_t* __restrict__ offsets) {
  __shared__ unsigned smem[CP_NT / 64 + 1];
  const long long base = (long long)blockIdx.x * CP_CHUNK + (long long)threadIdx.x * CP_ROWS_PER_THREAD;
  unsigned cv[CP_ROWS_PER_THREAD], c = 0;
#pragma unroll
  for (int k = 0; k < CP_ROWS_PER_THREAD; ++k) { cv[k] = base + k < N ? count_cursor[base + k] : 0u; c += cv[k]; }
  unsigned total;
  unsigned pos = block_sum[blockIdx.x] + block_excl_scan_u32<CP_NT>(c, &total, smem);
#pragma unroll
  for (int k = 0; k < CP_ROWS_PER_THREAD; ++k)
    if (base + k < N) { offsets[base + k] = (int32_t)pos; count_cursor[base + k] = pos; pos += cv[k]; }
}

__global__ void __launch_bounds__(MQ_THREADS)
mq_fill_kernel(MqGrid g, const float* __restrict__ vertices, const int32_t* __restrict__ faces, long long m, long long n,
               long long max_cells, uint32_t* cursor, int32_t* __restrict__ pairs, long long capacity, long long* state) {
  const long long t = (long long)blockIdx.x * MQ_THREADS + threadIdx.x;
  if (t == 0 && state[0] > capacity) mq_raise(state, MQ_ST_CAPACITY);
  if (t >= n) return;
  int lo[3], hi[3];
  long long cells;
  if (mq_classify(g, vertices, faces, t, m, max_cells, lo, hi, &cells) != MQ_SCATTERED) return;
  for (int z = lo[2]; z <= hi[2]; ++z)
    for (int y = lo[1]; y <= hi[1]; ++y)
      for (int x = lo[0]; x <= hi[0]; ++x) {
        const uint32_t pos = __hip_atomic_fetch_add(&cursor[mq_cell_index(g, x, y, z)], 1u, MQ_RLX);
        if ((long long)pos < capacity) pairs[pos] = (int32_t)t;
      }
}

// ---- the closest face ----------------------------------------------------------------------------------------------------------------
struct MqQuery {
  MqGrid g;
  long long m, n, npairs, k;
  double max_distance, max_d2;
};

struct MqBest { double d2, q[3]; int32_t face; };

__device__ __forceinline__ void mq_test_face(const MqQuery& Q, const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                             const double* p, long long t, MqBest* best, long long* state) {
  if (t < 0 || t >= Q.n) { mq_raise(state, MESH_ST_BAD_INDEX); return; }
  float a[3], b[3], c[3];
  if (!mq_load_face(vertices, faces, t, Q.m, a, b, c)) return;
  double q[3];
  const double d2 = mq_closest(p, a, b, c, q);
  if (mq_better(d2, (int32_t)t, best->d2, best->face)) { best->d2 = d2; best->face = (int32_t)t; best->q[0] = q[0]; best->q[1] = q[1]; best->q[2] = q[2]; }
}

__device__ __forceinline__ void mq_visit_cell(const MqQuery& Q, const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                              const int32_t* __restrict__ cell_start, const int32_t* __restrict__ pairs, const double* p,
                                              long long cell, int first, int step, MqBest* best, long long* state) {
  const long long lo = cell_start[cell], hi = cell_start[cell + 1];
  if (lo < 0 || hi < lo || hi > Q.npairs) { mq_raise(state, MESH_ST_BAD_INDEX); return; }
  for (long long j = lo + first; j < hi; j += step) mq_test_face(Q, vertices, faces, p, pairs[j], best, state);
}

// WAVE: a wave per query instead of a thread -- its lanes stride over the large list and over each cell's faces, the stop rule
// reads the wave's minimum d2 after every ring, and the lowest lane that holds the wave's minimum of (d2, face) writes the
// result. The same bytes. tools/variants/mesh_query_wave.patch builds that form (MQ_WAVE_PER_QUERY) for the A/B in
// profiles/r27_mesh_distance_ab.txt: a quarter faster against the 4 M-face mesh, 3 - 5.5 x slower on the other three workloads.
constexpr bool MQ_WAVE_PER_QUERY = false;

__device__ __forceinline__ double mq_wave_min(double v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) { const double o = __shfl_xor(v, d); v = o < v ? o : v; }
  return v;
}

template <typename PT, bool WAVE>
__global__ void __launch_bounds__(MQ_THREADS)
mq_closest_kernel(MqQuery Q, const float* __restrict__ vertices, const int32_t* __restrict__ faces, const int32_t* __restrict__ cell_start,
                  const int32_t* __restrict__ pairs, const int32_t* __restrict__ large, const long long* __restrict__ grid_state,
                  const PT* __restrict__ points, double* __restrict__ sqdist, int32_t* __restrict__ face_out, float* __restrict__ closest,
                  long long* state) {
  const long long tid = (long long)blockIdx.x * MQ_THREADS + threadIdx.x;
  const long long i = WAVE ? tid >> 6 : tid;
  const int first = WAVE ? (int)(threadIdx.x & 63u) : 0, step = WAVE ? 64 : 1;
  const bool active = i < Q.k;
  bool writer = !WAVE || first == 0;
  MqBest best;
  best.d2 = INFINITY; best.face = -1; best.q[0] = best.q[1] = best.q[2] = 0.0;
  if (tid == 0) state[3] = grid_state[3];                 // the faces the grid left out
  if (active) {
    const double p[3] = {(double)points[3 * i], (double)points[3 * i + 1], (double)points[3 * i + 2]};
    if (mq_finite(p[0]) && mq_finite(p[1]) && mq_finite(p[2])) {
      long long L = grid_state[1];
      if (L < 0 || L > Q.n) { mq_raise(state, MESH_ST_BAD_INDEX); L = 0; }
      for (long long j = first; j < L; j += step) mq_test_face(Q, vertices, faces, p, large[j], &best, state);
      long long q[3];
      int r0 = 0, r1 = 0;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const int qa = mq_query_cell(mq_cell(p[a], Q.g.origin[a], Q.g.cell));
        const int f = mq_ring_first(qa, Q.g.dims[a]), l = mq_ring_last(qa, Q.g.dims[a]);
        q[a] = qa; r0 = f > r0 ? f : r0; r1 = l > r1 ? l : r1;
      }
      // the stop rule holds from ring r0 on only: below it a face outside the grid, registered in a border cell, may lie right
      // next to a query outside the grid
      if (Q.npairs > 0) {
        for (long long r = r0; r <= r1; ++r) {          // r1 <= 2^30 + 2^28: the grid's farthest cell
          const long long lim[3] = {Q.g.dims[0] - 1, Q.g.dims[1] - 1, Q.g.dims[2] - 1};
          long long c0[3], c1[3];
#pragma unroll
          for (int a = 0; a < 3; ++a) { c0[a] = q[a] - r > 0 ? q[a] - r : 0; c1[a] = q[a] + r < lim[a] ? q[a] + r : lim[a]; }
          for (long long z = c0[2]; z <= c1[2]; ++z)
            for (long long y = c0[1]; y <= c1[1]; ++y) {
              const bool shell = z - q[2] == r || q[2] - z == r || y - q[1] == r || q[1] - y == r;
              if (shell) {
                for (long long x = c0[0]; x <= c1[0]; ++x)
                  mq_visit_cell(Q, vertices, faces, cell_start, pairs, p, mq_cell_index(Q.g, x, y, z), first, step, &best, state);
              } else {
                const long long xa = q[0] - r, xb = q[0] + r;
                if (xa >= 0 && xa <= lim[0]) mq_visit_cell(Q, vertices, faces, cell_start, pairs, p, mq_cell_index(Q.g, xa, y, z), first, step, &best, state);
                if (r > 0 && xb >= 0 && xb <= lim[0])
                  mq_visit_cell(Q, vertices, faces, cell_start, pairs, p, mq_cell_index(Q.g, xb, y, z), first, step, &best, state);
              }
            }
          const double reach = WAVE ? mq_wave_min(best.d2) : best.d2;      // (a d2 that won is finite or the starting +inf)
          if (reach < mq_ring_d2((int)r, Q.g.cell) || mq_ring_beyond((int)r, Q.g.cell, Q.max_distance)) break;
        }
      }
    }
    if (WAVE) {                                           // the wave's minimum of (d2, face); the lowest lane that holds it writes
      double gd2 = best.d2;
      int32_t gface = best.face;
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) {
        const double od2 = __shfl_xor(gd2, d);
        const int32_t oface = __shfl_xor(gface, d);
        if (oface >= 0 && mq_better(od2, oface, gd2, gface)) { gd2 = od2; gface = oface; }
      }
      const unsigned long long holders = __ballot(best.face == gface && (gface < 0 || best.d2 == gd2));
      writer = holders && (unsigned)first == (unsigned)__ffsll((unsigned long long)holders) - 1u;
    }
    if (best.face >= 0 && best.d2 > Q.max_d2) best.face = -1;
    if (best.face < 0) { best.d2 = INFINITY; best.q[0] = best.q[1] = best.q[2] = 0.0; }
    if (writer) { sqdist[i] = best.d2; face_out[i] = best.face; }
    if (writer && closest) store3(closest + 3 * i, (float)best.q[0], (float)best.q[1], (float)best.q[2]);
  }
  const unsigned lane = lane_id();
  const unsigned long long hit = __ballot(active && writer && best.face >= 0), miss = __ballot(active && writer && best.face < 0);
  if (lane == 0 && hit) __hip_atomic_fetch_add((unsigned long long*)&state[0], (unsigned long long)__popcll(hit), MQ_RLX);
  if (lane == 0 && miss) __hip_atomic_fetch_add((unsigned long long*)&state[1], (unsigned long long)__popcll(miss), MQ_RLX);
}

// ---- the summary of a query's distances ------------------------------------------------------------------------------------------
// ONE launch. Workgroup b takes queries b MQ_SUM_CHUNK ... in a fixed order (thread t its items t, t + 256, ..., then a tree over the
// threads in LDS) and leaves three float64 partials -- sum d, sum d2, max d over the answered queries -- and adds its integer
// counts to the output. The workgroup that draws the last ticket adds the partials in index order the same way: the sums are
// the same bytes run after run, whichever workgroup that is. No float atomics.
constexpr int MQ_SUM_CHUNK = 4096, MQ_MAX_THRESHOLDS = 16;
struct MqThresholds { double tau[MQ_MAX_THRESHOLDS]; int count; };

template <typename X, typename Op>
__device__ __forceinline__ X mq_block_reduce(X v, X* smem, Op op) {
  smem[threadIdx.x] = v;
  __syncthreads();
  for (int s = MQ_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) smem[threadIdx.x] = op(smem[threadIdx.x], smem[threadIdx.x + s]);
    __syncthreads();
  }
  const X r = smem[0];
  __syncthreads();
  return r;
}

__global__ void __launch_bounds__(MQ_THREADS)
mq_summary_kernel(const double* __restrict__ sqdist, const int32_t* __restrict__ face, long long k, MqThresholds T, long long NB,
                  unsigned long long* partials, unsigned* ticket, long long* out) {
  __shared__ double sd[MQ_THREADS];
  __shared__ unsigned long long sc[MQ_THREADS];
  __shared__ bool last;
  const auto add = [](double a, double b) { return a + b; };
  const auto mx = [](double a, double b) { return a > b ? a : b; };
  const auto addc = [](unsigned long long a, unsigned long long b) { return a + b; };
  double sum = 0.0, sum2 = 0.0, top = 0.0;
  unsigned long long cnt[MQ_MAX_THRESHOLDS + 1];
#pragma unroll
  for (int j = 0; j <= MQ_MAX_THRESHOLDS; ++j) cnt[j] = 0;
  const long long base = (long long)blockIdx.x * MQ_SUM_CHUNK;
  for (int it = 0; it < MQ_SUM_CHUNK / MQ_THREADS; ++it) {
    const long long i = base + (long long)it * MQ_THREADS + threadIdx.x;
    if (i < k && face[i] >= 0) {
      const double d2 = sqdist[i], d = sqrt(d2);
      sum = sum + d; sum2 = sum2 + d2; top = d > top ? d : top;
      ++cnt[0];
#pragma unroll
      for (int j = 0; j < MQ_MAX_THRESHOLDS; ++j) cnt[j + 1] += (j < T.count && d <= T.tau[j]) ? 1ull : 0ull;
    }
  }
  sum = mq_block_reduce(sum, sd, add); sum2 = mq_block_reduce(sum2, sd, add); top = mq_block_reduce(top, sd, mx);
#pragma unroll
  for (int j = 0; j <= MQ_MAX_THRESHOLDS; ++j) {
    if (j <= T.count) {                                   // uniform: every thread reaches the tree's barriers
      const unsigned long long c = mq_block_reduce(cnt[j], sc, addc);
      if (threadIdx.x == 0 && c) __hip_atomic_fetch_add((unsigned long long*)&out[3 + j], c, MQ_RLX);
    }
  }
  if (threadIdx.x == 0) {
    __hip_atomic_store(&partials[3 * blockIdx.x], (unsigned long long)__double_as_longlong(sum), MQ_RLX);
    __hip_atomic_store(&partials[3 * blockIdx.x + 1], (unsigned long long)__double_as_longlong(sum2), MQ_RLX);
    __hip_atomic_store(&partials[3 * blockIdx.x + 2], (unsigned long long)__double_as_longlong(top), MQ_RLX);
    __threadfence();
    last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(NB - 1);
  }
  __syncthreads();
  if (!last) return;
  __threadfence();
  sum = 0.0; sum2 = 0.0; top = 0.0;
  for (long long b = threadIdx.x; b < NB; b += MQ_THREADS) {
    const double a0 = __longlong_as_double((long long)__hip_atomic_load(&partials[3 * b], MQ_RLX));
    const double a1 = __longlong_as_double((long long)__hip_atomic_load(&partials[3 * b + 1], MQ_RLX));
    const double a2 = __longlong_as_double((long long)__hip_atomic_load(&partials[3 * b + 2], MQ_RLX));
    sum = sum + a0; sum2 = sum2 + a1; top = a2 > top ? a2 : top;
  }
  sum = mq_block_reduce(sum, sd, add); sum2 = mq_block_reduce(sum2, sd, add); top = mq_block_reduce(top, sd, mx);
  if (threadIdx.x == 0) { out[0] = __double_as_longlong(sum); out[1] = __double_as_longlong(sum2); out[2] = __double_as_longlong(top); }
}

// ---- the sampler -----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MQ_THREADS)
mq_sample_count_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces, long long m, long long n, double density,
                       uint32_t seed, uint32_t* __restrict__ count, long long* state) {
  const long long t = (long long)blockIdx.x * MQ_THREADS + threadIdx.x;
  long long cnt = 0;
  if (t < n) {
    float a[3], b[3], c[3];
    if (!mq_load_face(vertices, faces, t, m, a, b, c)) mq_raise(state, MESH_ST_BAD_INDEX);
    else {
      cnt = mq_sample_count(mq_area(a, b, c), density, seed, (uint32_t)t);
      if (cnt < 0) { cnt = 0; mq_raise(state, MQ_ST_BAD_FACE); }
    }
    count[t] = (uint32_t)cnt;
  }
  const unsigned long long sum = mq_wave_sum((unsigned long long)cnt);
  if (lane_id() == 0 && sum) __hip_atomic_fetch_add((unsigned long long*)&state[0], sum, MQ_RLX);
}

__global__ void __launch_bounds__(MQ_THREADS)
mq_sample_emit_kernel(const float* __restrict__ vertices, const float* __restrict__ colors, const int32_t* __restrict__ faces, long long m,
                      long long n, uint32_t seed, const int32_t* __restrict__ offsets, long long capacity, float* __restrict__ points,
                      int32_t* __restrict__ face_out, float* __restrict__ colors_out) {
  const long long t = (long long)blockIdx.x * MQ_THREADS + threadIdx.x;
  if (t >= n) return;
  const long long lo = offsets[t], cnt = (long long)offsets[t + 1] - lo;
  if (lo < 0 || cnt <= 0 || cnt > MQ_MAX_SAMPLES_PER_FACE) return;
  const int32_t ia = faces[3 * t], ib = faces[3 * t + 1], ic = faces[3 * t + 2];
  if (!(mesh_index_ok(ia, m) && mesh_index_ok(ib, m) && mesh_index_ok(ic, m))) return;      // its count is 0: never
  float a[3], b[3], c[3], ca[3] = {0.f, 0.f, 0.f}, cb[3] = {0.f, 0.f, 0.f}, cc[3] = {0.f, 0.f, 0.f};
  load3(vertices + 3ll * ia, a); load3(vertices + 3ll * ib, b); load3(vertices + 3ll * ic, c);
  if (colors_out) { load3(colors + 3ll * ia, ca); load3(colors + 3ll * ib, cb); load3(colors + 3ll * ic, cc); }
  for (long long j = 0; j < cnt; ++j) {
    const long long row = lo + j;
    if (row >= capacity) return;
    double u1, u2;
    mq_sample_uv(seed, (uint32_t)t, (uint32_t)j, &u1, &u2);
    store3(points + 3 * row, mq_sample_attr(a[0], b[0], c[0], u1, u2), mq_sample_attr(a[1], b[1], c[1], u1, u2),
           mq_sample_attr(a[2], b[2], c[2], u1, u2));
    face_out[row] = (int32_t)t;
    if (colors_out)
      store3(colors_out + 3 * row, mq_sample_attr(ca[0], cb[0], cc[0], u1, u2), mq_sample_attr(ca[1], cb[1], cc[1], u1, u2),
             mq_sample_attr(ca[2], cb[2], cc[2], u1, u2));
  }
}

}  // namespace sfgs

using namespace sfgs;

namespace {

struct MqScanScratch {
  uint32_t* cursor;                   // [N] the counts, then the fill's cursors
  unsigned* block_sum;                // [cp_blocks(N)]
  int32_t* offsets;                   // [N + 1], the sampler's only: the grid's offsets are its cell_start
  size_t total;
};
MqScanScratch mq_scan_view(void* base, long long N, bool with_offsets) {
  MqScanScratch s;
  char* p = (char*)base;
  size_t off = 0;
  s.cursor = (uint32_t*)(p + off); off += align_up((size_t)N * 4 + 4, 256);
  s.block_sum = (unsigned*)(p + off); off += align_up((size_t)cp_blocks(N) * 4 + 4, 256);
  s.offsets = (int32_t*)(p + off); off += with_offsets ? align_up((size_t)N * 4 + 4, 256) : 0;
  s.total = off;
  return s;
}

int mq_scan(const MqScanScratch& s, long long N, int32_t* offsets, long long* state, hipStream_t stream) {
  const long long NB = cp_blocks(N);
  hipLaunchKernelGGL(mq_chunk_sum_kernel, dim3((unsigned)NB), dim3(CP_NT), 0, stream, (const uint32_t*)s.cursor, N, s.block_sum);
  hipLaunchKernelGGL(mq_scan_top_kernel, dim3(1), dim3(SCAN_TOP_THREADS), 0, stream, s.block_sum, NB, offsets + N, state);
  hipLaunchKernelGGL(mq_offsets_kernel, dim3((unsigned)NB), dim3(CP_NT), 0, stream, s.cursor, N, (const unsigned*)s.block_sum, offsets);
  SFGS_POST_LAUNCH("mq_scan", stream, 0);
  return SFGS_OK;
}

inline unsigned mq_blocks(long long items) { return (unsigned)((items + MQ_THREADS - 1) / MQ_THREADS); }

int mq_check_mesh(const char* what, int64_t m, int64_t n, const void* vertices, const void* faces) {
  SFGS_REQUIRE(n >= 0 && n <= MESH_MAX_TRIANGLES, SFGS_E_ARG, "%s: n = %lld outside 0 ... 2^29", what, (long long)n);
  SFGS_REQUIRE(m >= 0 && m <= MESH_MAX_VERTICES, SFGS_E_ARG, "%s: m = %lld outside 0 ... 2^31 - 1", what, (long long)m);
  SFGS_REQUIRE(m > 0 || n == 0, SFGS_E_ARG, "%s: %lld faces over no vertex", what, (long long)n);
  SFGS_REQUIRE(m == 0 || vertices, SFGS_E_ARG, "%s: NULL vertices", what);
  SFGS_REQUIRE(n == 0 || faces, SFGS_E_ARG, "%s: NULL faces", what);
  return SFGS_OK;
}

long long mq_grid_cells(const SfgsMeshGrid* a) {       // 0: not a grid
  if (a->nx < 1 || a->ny < 1 || a->nz < 1) return 0;
  const long long xy = (long long)a->nx * a->ny;
  if (xy > MQ_MAX_GRID_CELLS || xy * a->nz > MQ_MAX_GRID_CELLS) return 0;
  return xy * a->nz;
}

int mq_check_grid(const char* what, const SfgsMeshGrid* a, MqGrid* g, long long* max_cells) {
  SFGS_REQUIRE(a, SFGS_E_ARG, "%s: NULL SfgsMeshGrid", what);
  SFGS_REQUIRE(a->struct_size == sizeof(SfgsMeshGrid), SFGS_E_ARG, "%s: SfgsMeshGrid.struct_size %u, expected %zu", what, a->struct_size,
               sizeof(SfgsMeshGrid));
  if (const int rc = mq_check_mesh(what, a->m, a->n, a->vertices, a->faces)) return rc;
  SFGS_REQUIRE(mq_grid_cells(a) > 0, SFGS_E_ARG, "%s: %d x %d x %d cells: every dimension >= 1, at most 2^28 cells in all", what, a->nx,
               a->ny, a->nz);
  SFGS_REQUIRE(a->cell > 0.0 && a->cell - a->cell == 0.0, SFGS_E_ARG, "%s: cell %g, finite and > 0", what, a->cell);
  for (int k = 0; k < 3; ++k)
    SFGS_REQUIRE(a->origin[k] - a->origin[k] == 0.0, SFGS_E_ARG, "%s: origin[%d] %g is not finite", what, k, a->origin[k]);
  SFGS_REQUIRE(a->max_cells >= -1 && a->max_cells <= MQ_MAX_CELLS_LIMIT, SFGS_E_ARG, "%s: max_cells %lld: -1 (default) ... 2^30", what,
               (long long)a->max_cells);
  SFGS_REQUIRE(a->capacity >= 0 && a->capacity <= 0x7fffffffll, SFGS_E_ARG, "%s: capacity %lld outside 0 ... 2^31 - 1", what,
               (long long)a->capacity);
  SFGS_REQUIRE(a->cell_start && a->state, SFGS_E_ARG, "%s: NULL cell_start or state", what);
  SFGS_REQUIRE(a->n == 0 || a->large, SFGS_E_ARG, "%s: NULL large list", what);
  for (int k = 0; k < 3; ++k) g->origin[k] = a->origin[k];
  g->cell = a->cell; g->dims[0] = a->nx; g->dims[1] = a->ny; g->dims[2] = a->nz;
  *max_cells = a->max_cells < 0 ? MQ_MAX_CELLS_DEFAULT : a->max_cells;
  return SFGS_OK;
}

}  // namespace

extern "C" size_t sfgs_mesh_grid_scratch_bytes(int32_t nx, int32_t ny, int32_t nz) {
  SfgsMeshGrid a = {};
  a.nx = nx; a.ny = ny; a.nz = nz;
  const long long cells = mq_grid_cells(&a);
  if (cells == 0) {
    sfgs::set_error("sfgs_mesh_grid_scratch_bytes: %d x %d x %d cells: every dimension >= 1, at most 2^28 cells in all", nx, ny, nz);
    return 0;
  }
  return mq_scan_view(nullptr, cells, false).total;
}

extern "C" int sfgs_mesh_grid_count(const SfgsMeshGrid* a, void* scratch, size_t scratch_bytes, void* stream_) {
  MqGrid g;
  long long max_cells;
  if (const int rc = mq_check_grid("sfgs_mesh_grid_count", a, &g, &max_cells)) return rc;
  SFGS_REQUIRE(scratch, SFGS_E_ARG, "sfgs_mesh_grid_count: NULL scratch");
  const long long cells = mq_grid_cells(a);
  const MqScanScratch s = mq_scan_view(scratch, cells, false);
  SFGS_REQUIRE(scratch_bytes >= s.total, SFGS_E_ARG, "mesh grid scratch too small: %zu < %zu", scratch_bytes, s.total);
  hipStream_t stream = (hipStream_t)stream_;
  SFGS_CHECK_HIP(hipMemsetAsync(a->state, 0, 32, stream));
  if (a->n == 0) {                                       // every cell is empty
    SFGS_CHECK_HIP(hipMemsetAsync(a->cell_start, 0, ((size_t)cells + 1) * 4, stream));
    return SFGS_OK;
  }
  SFGS_CHECK_HIP(hipMemsetAsync(s.cursor, 0, (size_t)cells * 4, stream));
  hipLaunchKernelGGL(mq_count_kernel, dim3(mq_blocks(a->n)), dim3(MQ_THREADS), 0, stream, g, a->vertices, a->faces, (long long)a->m,
                     (long long)a->n, max_cells, s.cursor, a->large, a->state);
  SFGS_POST_LAUNCH("mq_count", stream, 0);
  return mq_scan(s, cells, a->cell_start, a->state, stream);
}

extern "C" int sfgs_mesh_grid_fill(const SfgsMeshGrid* a, void* scratch, size_t scratch_bytes, void* stream_) {
  MqGrid g;
  long long max_cells;
  if (const int rc = mq_check_grid("sfgs_mesh_grid_fill", a, &g, &max_cells)) return rc;
  SFGS_REQUIRE(scratch, SFGS_E_ARG, "sfgs_mesh_grid_fill: NULL scratch");
  SFGS_REQUIRE(a->capacity == 0 || a->pairs, SFGS_E_ARG, "sfgs_mesh_grid_fill: NULL pairs");
  const long long cells = mq_grid_cells(a);
  const MqScanScratch s = mq_scan_view(scratch, cells, false);
  SFGS_REQUIRE(scratch_bytes >= s.total, SFGS_E_ARG, "mesh grid scratch too small: %zu < %zu", scratch_bytes, s.total);
  hipStream_t stream = (hipStream_t)stream_;
  if (a->n == 0) return SFGS_OK;
  hipLaunchKernelGGL(mq_fill_kernel, dim3(mq_blocks(a->n)), dim3(MQ_THREADS), 0, stream, g, a->vertices, a->faces, (long long)a->m,
                     (long long)a->n, max_cells, s.cursor, a->pairs, (long long)a->capacity, a->state);
  SFGS_POST_LAUNCH("mq_fill", stream, 0);
  if (a->capacity > 0) {
    hipLaunchKernelGGL(vf_sort_kernel, dim3(mq_blocks(cells)), dim3(MQ_THREADS), 0, stream, (const int32_t*)a->cell_start, cells,
                       (long long)a->capacity, a->pairs, a->state);
    SFGS_POST_LAUNCH("mq_sort", stream, 0);
  }
  return SFGS_OK;
}

extern "C" int sfgs_mesh_closest(const SfgsMeshGrid* a, const void* points, int32_t points_f64, int64_t k, double max_distance,
                                 double* sqdist, int32_t* face, float* closest, long long* state, void* stream_) {
  MqQuery Q;
  long long max_cells;
  if (const int rc = mq_check_grid("sfgs_mesh_closest", a, &Q.g, &max_cells)) return rc;
  SFGS_REQUIRE(a->capacity == 0 || a->pairs, SFGS_E_ARG, "sfgs_mesh_closest: NULL pairs");
  SFGS_REQUIRE(k >= 0 && k <= 0x7fffffffll, SFGS_E_ARG, "sfgs_mesh_closest: k = %lld outside 0 ... 2^31 - 1", (long long)k);
  SFGS_REQUIRE(points_f64 == 0 || points_f64 == 1, SFGS_E_ARG, "sfgs_mesh_closest: points_f64 %d: 0 (float32) or 1 (float64)", points_f64);
  SFGS_REQUIRE(max_distance >= 0.0, SFGS_E_ARG, "sfgs_mesh_closest: max_distance %g: >= 0 (+inf: none)", max_distance);      // NaN fails
  SFGS_REQUIRE(state, SFGS_E_ARG, "sfgs_mesh_closest: NULL state");
  SFGS_REQUIRE(k == 0 || (points && sqdist && face), SFGS_E_ARG, "sfgs_mesh_closest: NULL points, sqdist or face");
  hipStream_t stream = (hipStream_t)stream_;
  SFGS_CHECK_HIP(hipMemsetAsync(state, 0, 32, stream));
  if (k == 0) {                                          // the grid's faces left out, as a launch would report them
    SFGS_CHECK_HIP(hipMemcpyAsync(state + 3, a->state + 3, sizeof(long long), hipMemcpyDeviceToDevice, stream));
    return SFGS_OK;
  }
  Q.m = a->m; Q.n = a->n; Q.npairs = a->capacity; Q.k = k;
  Q.max_distance = max_distance; Q.max_d2 = max_distance * max_distance;
  const long long threads = MQ_WAVE_PER_QUERY ? (long long)k * 64 : (long long)k;
  if (points_f64)
    hipLaunchKernelGGL((mq_closest_kernel<double, MQ_WAVE_PER_QUERY>), dim3(mq_blocks(threads)), dim3(MQ_THREADS), 0, stream, Q, a->vertices, a->faces,
                       (const int32_t*)a->cell_start, (const int32_t*)a->pairs, (const int32_t*)a->large, (const long long*)a->state,
                       (const double*)points, sqdist, face, closest, state);
  else
    hipLaunchKernelGGL((mq_closest_kernel<float, MQ_WAVE_PER_QUERY>), dim3(mq_blocks(threads)), dim3(MQ_THREADS), 0, stream, Q, a->vertices, a->faces,
                       (const int32_t*)a->cell_start, (const int32_t*)a->pairs, (const int32_t*)a->large, (const long long*)a->state,
                       (const float*)points, sqdist, face, closest, state);
  SFGS_POST_LAUNCH("mq_closest", stream, 0);
  return SFGS_OK;
}

extern "C" size_t sfgs_mesh_distance_summary_scratch_bytes(int64_t k) {
  if (k < 0 || k > 0x7fffffffll) {
    sfgs::set_error("sfgs_mesh_distance_summary_scratch_bytes: k = %lld outside 0 ... 2^31 - 1", (long long)k);
    return 0;
  }
  return 256 + align_up((size_t)((k + MQ_SUM_CHUNK - 1) / MQ_SUM_CHUNK) * 24 + 24, 256);
}

extern "C" int sfgs_mesh_distance_summary(const double* sqdist, const int32_t* face, int64_t k, const double* thresholds,
                                          int32_t num_thresholds, long long* out, void* scratch, size_t scratch_bytes, void* stream_) {
  SFGS_REQUIRE(k >= 0 && k <= 0x7fffffffll, SFGS_E_ARG, "sfgs_mesh_distance_summary: k = %lld outside 0 ... 2^31 - 1", (long long)k);
  SFGS_REQUIRE(num_thresholds >= 0 && num_thresholds <= MQ_MAX_THRESHOLDS, SFGS_E_ARG,
               "sfgs_mesh_distance_summary: %d thresholds, 0 ... 16", num_thresholds);
  SFGS_REQUIRE(num_thresholds == 0 || thresholds, SFGS_E_ARG, "sfgs_mesh_distance_summary: NULL thresholds");
  MqThresholds T;
  T.count = num_thresholds;
  for (int j = 0; j < MQ_MAX_THRESHOLDS; ++j) T.tau[j] = j < num_thresholds ? thresholds[j] : 0.0;
  for (int j = 0; j < num_thresholds; ++j)
    SFGS_REQUIRE(T.tau[j] >= 0.0, SFGS_E_ARG, "sfgs_mesh_distance_summary: threshold %d is %g: >= 0", j, T.tau[j]);      // NaN fails
  SFGS_REQUIRE(out && scratch, SFGS_E_ARG, "sfgs_mesh_distance_summary: NULL out or scratch");
  SFGS_REQUIRE(k == 0 || (sqdist && face), SFGS_E_ARG, "sfgs_mesh_distance_summary: NULL sqdist or face");
  const size_t need = sfgs_mesh_distance_summary_scratch_bytes(k);
  SFGS_REQUIRE(scratch_bytes >= need, SFGS_E_ARG, "mesh distance summary scratch too small: %zu < %zu", scratch_bytes, need);
  hipStream_t stream = (hipStream_t)stream_;
  SFGS_CHECK_HIP(hipMemsetAsync(out, 0, (4 + MQ_MAX_THRESHOLDS) * sizeof(long long), stream));
  if (k == 0) return SFGS_OK;
  SFGS_CHECK_HIP(hipMemsetAsync(scratch, 0, 256, stream));
  const long long NB = (k + MQ_SUM_CHUNK - 1) / MQ_SUM_CHUNK;
  hipLaunchKernelGGL(mq_summary_kernel, dim3((unsigned)NB), dim3(MQ_THREADS), 0, stream, sqdist, face, (long long)k, T, NB,
                     (unsigned long long*)((char*)scratch + 256), (unsigned*)scratch, out);
  SFGS_POST_LAUNCH("mq_summary", stream, 0);
  return SFGS_OK;
}

extern "C" size_t sfgs_mesh_sample_scratch_bytes(int64_t n) {
  if (n < 0 || n > MESH_MAX_TRIANGLES) {
    sfgs::set_error("sfgs_mesh_sample_scratch_bytes: %lld faces, 0 ... 2^29", (long long)n);
    return 0;
  }
  return mq_scan_view(nullptr, n, true).total;
}

extern "C" int sfgs_mesh_sample(const float* vertices, const float* colors, const int32_t* faces, int64_t m, int64_t n, double density,
                                uint32_t seed, int64_t capacity, float* points, int32_t* face, float* colors_out, long long* state,
                                void* scratch, size_t scratch_bytes, void* stream_) {
  if (const int rc = mq_check_mesh("sfgs_mesh_sample", m, n, vertices, faces)) return rc;
  SFGS_REQUIRE(density >= 0.0 && density - density == 0.0, SFGS_E_ARG, "sfgs_mesh_sample: density %g, finite and >= 0", density);
  SFGS_REQUIRE(capacity >= 0 && capacity <= 0x7fffffffll, SFGS_E_ARG, "sfgs_mesh_sample: capacity %lld outside 0 ... 2^31 - 1",
               (long long)capacity);
  SFGS_REQUIRE(state && scratch, SFGS_E_ARG, "sfgs_mesh_sample: NULL state or scratch");
  SFGS_REQUIRE(capacity == 0 || (points && face), SFGS_E_ARG, "sfgs_mesh_sample: NULL points or face");
  SFGS_REQUIRE(!colors_out || colors, SFGS_E_ARG, "sfgs_mesh_sample: colors_out without colors");
  const MqScanScratch s = mq_scan_view(scratch, n, true);
  SFGS_REQUIRE(scratch_bytes >= s.total, SFGS_E_ARG, "mesh sample scratch too small: %zu < %zu", scratch_bytes, s.total);
  hipStream_t stream = (hipStream_t)stream_;
  SFGS_CHECK_HIP(hipMemsetAsync(state, 0, 32, stream));
  if (n == 0) return SFGS_OK;
  const dim3 grid(mq_blocks(n)), block(MQ_THREADS);
  hipLaunchKernelGGL(mq_sample_count_kernel, grid, block, 0, stream, vertices, faces, (long long)m, (long long)n, density, seed, s.cursor,
                     state);
  SFGS_POST_LAUNCH("mq_sample_count", stream, 0);
  if (const int rc = mq_scan(s, n, s.offsets, state, stream)) return rc;
  if (capacity > 0) {
    hipLaunchKernelGGL(mq_sample_emit_kernel, grid, block, 0, stream, vertices, colors_out ? colors : nullptr, faces, (long long)m,
                       (long long)n, seed, (const int32_t*)s.offsets, (long long)capacity, points, face, colors_out);
    SFGS_POST_LAUNCH("mq_sample_emit", stream, 0);
  }
  return SFGS_OK;
}
