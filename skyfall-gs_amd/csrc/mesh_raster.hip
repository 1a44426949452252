// mesh_raster.hip -- an indexed triangle mesh seen from a camera (sfgs_mesh_render; Python: Mesh.render): depth along the forward
// axis, the index of the visible face, its normal and its colour, per pixel. include/sfgs.h states the result in words,
// tests/mesh_render_np.py in numpy, mesh_raster_math.h holds every per-element function; the kernels equal the restatement byte
// for byte, whatever the order of arrival, the route a face takes or the launch shape: coverage is decided in int64 on
// snapped vertices and a pixel's winner is the minimum of a 64-bit key (float32 depth bits << 32 | face index).
//   1. mr_project_kernel   a thread per vertex writes its 16-byte record (X, Y, z; X == INT32_MIN: unusable). A face gathers
//                          three records instead of projecting every vertex about six times.
//   2. mr_face_kernel      a thread per face: set-up, the box of pixels clipped to the image. A box of at most small_max pixels
//                          is walked by the thread itself; a larger face is appended to one of two lists of face indices -- LARGE
//                          (its box touches at most MR_HUGE_TILES 8 x 8 tiles) or HUGE -- with ONE counter atomic per wave and
//                          list. The four counts are summed per wave and added to one of MR_COUNT_LINES sets of counters, each
//                          on a cache line of its own: four counters for all 62 000 waves of a 4 M-face mesh serialised on
//                          their lines and took 0.8 of the kernel's 0.81 ms (profiles/r26_mesh_render_ab.txt).
//   3. mr_large_kernel     a fixed grid of waves strides over the items: a LARGE face is one item, a HUGE face MR_BANDS items,
//                          each a run of its tiles in row-major order, so one face that fills the frame is spread over MR_BANDS
//                          waves. A wave takes an 8 x 8 tile of pixels with a lane per pixel and rejects a tile that lies wholly
//                          outside one edge before testing pixels. The lists' lengths stay on the device. Each list holds n
//                          entries and a face is appended at most once: they cannot overflow.
//   4. mr_resolve_kernel   a thread per pixel, a wave an 8 x 8 tile: decodes the key, gathers the winner's records again,
//                          recomputes the weights with the shared functions and writes depth, face, normal, rgb. Its first wave
//                          also sums the sets of counters into the state.
// The pixel keys are touched by relaxed agent-scope atomicMin and, in resolve, by plain loads after the kernel boundary. (A
// relaxed load in front that skips the atomic when the stored key is already smaller -- the move that saved ortho.hip's
// accumulate kernel 24 % -- LOSES here, where few faces meet on a pixel: the atomic returns nothing and is not waited for, the
// load is; MR_LOAD_FIRST below, measured in profiles/r26_mesh_render_ab.txt.) Every loop is bounded by the box of a face, by
// small_max or by the lists' lengths; every index is checked before its use: a face's three against m (a bad one is not drawn,
// counts as clipped and raises status bit 3), a pixel against the clipped box, a winner's face against n. No float atomics, no
// LDS, no barrier. No profiler ids.
#include "sfgs_internal.h"
#include "mesh_raster_math.h"

namespace sfgs {

constexpr int MR_THREADS = 256;
constexpr int MR_TILE = 16;                 // resolve: a workgroup is 16 x 16 pixels, a wave 8 x 8
constexpr int MR_LARGE_BLOCKS = 1024;       // the large route's fixed grid
constexpr long long MR_SMALL_MAX_DEFAULT = 64;    // from the sweep in profiles/r26_mesh_render_ab.txt
constexpr int MR_HUGE_TILES = 64;           // a listed face whose box touches more tiles than this is dealt to MR_BANDS waves
constexpr int MR_BANDS = 256;
constexpr int MR_COUNT_LINES = 256, MR_COUNT_STRIDE = 16;      // sets of counters, 128 bytes apart
// a load in front of the pixel's atomicMin that skips it when the stored key is already smaller (keys only fall, so a stale value
// would cost an atomic, never a result); true: tools/variants/mesh_raster_load_first.patch builds that form for the A/B in
// profiles/r26_mesh_render_ab.txt
constexpr bool MR_LOAD_FIRST = false;
enum { MR_STATE_STATUS = 4 };               // state words 0 ... 3 are the counts
// status bit 0: a list of larger faces was asked for more than its n entries, or held an index >= n. A face is appended at most
// once, so valid kernels never raise it; if it is ever raised a face was left out, and check() says so instead of a silent hole.
constexpr unsigned MR_ST_LIST = MESH_ST_PROBE_BOUND;

__device__ __forceinline__ void mr_raise(long long* state, unsigned bits) {
  __hip_atomic_fetch_or((unsigned long long*)&state[MR_STATE_STATUS], (unsigned long long)bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

#define MR_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

struct MrParams {
  GeoCamera cam;
  double near, far;
  int H, W, camera_sign, cull;
  long long m, n, small_max;
};

__device__ __forceinline__ void mr_pixel(const MrFace& f, const long long* E, uint32_t face, double far, long long p,
                                         unsigned long long* keys) {
  double q[3], s;
  const float d = mr_depth(f, E, q, &s);
  if (!mr_depth_kept(d, far)) return;
  const unsigned long long key = mr_key(d, face);
  if (MR_LOAD_FIRST && __hip_atomic_load(&keys[p], MR_RLX) <= key) return;
  __hip_atomic_fetch_min(&keys[p], key, MR_RLX);
}

__device__ __forceinline__ bool mr_load_face(const MrParams& P, const MrVertex* __restrict__ rec, const int32_t* __restrict__ faces,
                                             long long t, MrFace* f, int* outcome) {
  const int32_t ia = faces[3 * t], ib = faces[3 * t + 1], ic = faces[3 * t + 2];
  if (!(mesh_index_ok(ia, P.m) && mesh_index_ok(ib, P.m) && mesh_index_ok(ic, P.m))) { *outcome = MR_CLIPPED; return false; }
  *outcome = mr_face_setup(rec[ia], rec[ib], rec[ic], P.camera_sign, P.cull, f);
  return true;
}

__global__ void __launch_bounds__(MR_THREADS)
mr_project_kernel(MrParams P, const float* __restrict__ vertices, MrVertex* __restrict__ rec) {
  const long long v = (long long)blockIdx.x * MR_THREADS + threadIdx.x;
  if (v >= P.m) return;
  float p[3];
  load3(vertices + 3 * v, p);
  rec[v] = mr_project(P.cam, p, P.near);
}

__global__ void __launch_bounds__(MR_THREADS)
mr_face_kernel(MrParams P, const MrVertex* __restrict__ rec, const int32_t* __restrict__ faces, unsigned long long* keys,
               uint32_t* __restrict__ list_large, uint32_t* __restrict__ list_huge, unsigned long long* list_count,
               unsigned long long* count_lines, long long* state) {
  const long long t = (long long)blockIdx.x * MR_THREADS + threadIdx.x;
  int outcome = -1;
  bool large = false, huge = false, bad = false;
  int c0 = 0, c1 = 0, r0 = 0, r1 = 0;
  if (t < P.n) {
    MrFace f;
    bad = !mr_load_face(P, rec, faces, t, &f, &outcome);
    if (outcome == MR_DRAWN && mr_box(f, P.H, P.W, &c0, &c1, &r0, &r1)) {
      const long long bw = c1 - c0 + 1, bh = r1 - r0 + 1;
      if (bw * bh <= P.small_max) {
        long long dx[3], dy[3], Erow[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) { mr_edge_dir(f, i, &dx[i], &dy[i]); Erow[i] = mr_edge_at(f, i, c0, r0); }
        for (int row = r0; row <= r1; ++row) {
          long long E[3] = {Erow[0], Erow[1], Erow[2]};
          for (int col = c0; col <= c1; ++col) {
            if (mr_edge_inside(E[0], dx[0], dy[0]) && mr_edge_inside(E[1], dx[1], dy[1]) && mr_edge_inside(E[2], dx[2], dy[2]))
              mr_pixel(f, E, (uint32_t)t, P.far, (long long)row * P.W + col, keys);
#pragma unroll
            for (int i = 0; i < 3; ++i) E[i] -= dy[i] * 256;       // one pixel to the right
          }
#pragma unroll
          for (int i = 0; i < 3; ++i) Erow[i] += dx[i] * 256;      // one pixel down
        }
      } else {
        huge = (long long)((c1 >> 3) - (c0 >> 3) + 1) * ((r1 >> 3) - (r0 >> 3) + 1) > MR_HUGE_TILES;
        large = !huge;
      }
    }
  }
  // the counts, one atomic per wave and category, into the workgroup's set of counters
  const unsigned lane = lane_id();
  unsigned long long* counters = count_lines + (size_t)(blockIdx.x % MR_COUNT_LINES) * MR_COUNT_STRIDE;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned long long b = __ballot(outcome == k);
    if (b && lane == 0) __hip_atomic_fetch_add(&counters[k], (unsigned long long)__popcll(b), MR_RLX);
  }
  if (__ballot(bad) && lane == 0) __hip_atomic_fetch_or((unsigned long long*)&state[MR_STATE_STATUS], (unsigned long long)MESH_ST_BAD_INDEX, MR_RLX);
  // the listed faces: one counter atomic per wave and list, the lanes' places from the ballot
#pragma unroll
  for (int which = 0; which < 2; ++which) {
    const bool mine = which ? huge : large;
    const unsigned long long lb = __ballot(mine);
    if (!lb) continue;
    unsigned long long base = 0;
    if (lane == 0) base = __hip_atomic_fetch_add(&list_count[which], (unsigned long long)__popcll(lb), MR_RLX);
    base = __shfl(base, 0);
    if (mine) {
      const unsigned long long at = base + (unsigned long long)__popcll(lb & ((1ull << lane) - 1ull));
      if (at < (unsigned long long)P.n) (which ? list_huge : list_large)[at] = (uint32_t)t;      // always: a face is appended at most once
      else mr_raise(state, MR_ST_LIST);
    }
  }
}

__global__ void __launch_bounds__(MR_THREADS)
mr_large_kernel(MrParams P, const MrVertex* __restrict__ rec, const int32_t* __restrict__ faces, unsigned long long* keys,
                const uint32_t* __restrict__ list_large, const uint32_t* __restrict__ list_huge,
                const unsigned long long* __restrict__ list_count, long long* state) {
  const unsigned lane = threadIdx.x & 63u;
  const long long wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (MR_THREADS / 64) + (threadIdx.x >> 6)));
  const long long waves = (long long)gridDim.x * (MR_THREADS / 64);
  unsigned long long L1 = list_count[0], L2 = list_count[1];
  if (L1 > (unsigned long long)P.n || L2 > (unsigned long long)P.n) {      // never; mr_face_kernel has raised the status already
    if (lane == 0) mr_raise(state, MR_ST_LIST);
    L1 = L1 > (unsigned long long)P.n ? (unsigned long long)P.n : L1;
    L2 = L2 > (unsigned long long)P.n ? (unsigned long long)P.n : L2;
  }
  const long long items = (long long)L1 + (long long)L2 * MR_BANDS;
  for (long long item = wave; item < items; item += waves) {
    const bool whole = item < (long long)L1;
    const long long j = item - (long long)L1;
    const long long t = whole ? list_large[item] : list_huge[j / MR_BANDS];
    const long long band = whole ? 0 : j % MR_BANDS;
    if (t >= P.n) {                                     // never: the lists hold what mr_face_kernel wrote
      if (lane == 0) mr_raise(state, MR_ST_LIST);
      continue;
    }
    MrFace f;
    int outcome, c0, c1, r0, r1;
    if (!mr_load_face(P, rec, faces, t, &f, &outcome) || outcome != MR_DRAWN || !mr_box(f, P.H, P.W, &c0, &c1, &r0, &r1)) continue;
    const int tx0 = c0 >> 3, ty0 = r0 >> 3, tcols = (c1 >> 3) - tx0 + 1;
    const long long tiles = (long long)tcols * ((r1 >> 3) - ty0 + 1);           // <= 2^24: H W <= 2^30
    const long long first = whole ? 0 : tiles * band / MR_BANDS, last = whole ? tiles : tiles * (band + 1) / MR_BANDS;
    long long dx[3], dy[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) mr_edge_dir(f, i, &dx[i], &dy[i]);
    for (long long ti = first; ti < last; ++ti) {       // this item's run of the box's tiles, row-major
      const int ty = ty0 + (int)(ti / tcols), tx = tx0 + (int)(ti % tcols);
      const int ra = ty * 8 > r0 ? ty * 8 : r0, rb = ty * 8 + 7 < r1 ? ty * 8 + 7 : r1;
      const int ca = tx * 8 > c0 ? tx * 8 : c0, cb = tx * 8 + 7 < c1 ? tx * 8 + 7 : c1;
      bool out = false;
#pragma unroll
      for (int i = 0; i < 3; ++i)                       // the edge's largest value over the tile's pixels
        out = out || mr_edge_at(f, i, dy[i] > 0 ? ca : cb, dx[i] > 0 ? rb : ra) < 0;
      if (out) continue;
      const int col = tx * 8 + (int)(lane & 7u), row = ty * 8 + (int)(lane >> 3);
      if (col < ca || col > cb || row < ra || row > rb) continue;         // no barrier follows
      long long E[3];
      if (mr_covers(f, col, row, E)) mr_pixel(f, E, (uint32_t)t, P.far, (long long)row * P.W + col, keys);
    }
  }
}

// NORMALS: 0 none, 1 flat, 2 interpolated vertex normals
template <int NORMALS, bool COLORS>
__global__ void __launch_bounds__(MR_THREADS)
mr_resolve_kernel(MrParams P, const MrVertex* __restrict__ rec, const int32_t* __restrict__ faces, const float* __restrict__ vertices,
                  const float* __restrict__ colors, const float* __restrict__ vnormals, const unsigned long long* __restrict__ keys,
                  float* __restrict__ depth, int32_t* __restrict__ face_out, float* __restrict__ normal, float* __restrict__ rgb,
                  const unsigned long long* __restrict__ count_lines, long long* state) {
  const unsigned tiles_x = (unsigned)((P.W + MR_TILE - 1) / MR_TILE);
  const unsigned tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
  const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  if (blockIdx.x == 0 && wave == 0) {                   // the counts: the sets of counters summed, state words 0 ... 3
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      unsigned long long sum = 0;
      for (int l = (int)lane; l < MR_COUNT_LINES; l += 64) sum += count_lines[l * MR_COUNT_STRIDE + k];
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d);
      if (lane == 0) state[k] = (long long)sum;
    }
  }
  const int col = (int)(tile_x * MR_TILE + (wave & 1u) * 8u + (lane & 7u));
  const int row = (int)(tile_y * MR_TILE + (wave >> 1) * 8u + (lane >> 3));
  if (row >= P.H || col >= P.W) return;                 // before any load; no barrier follows
  const long long N = (long long)P.H * P.W, p = (long long)row * P.W + col;
  const unsigned long long key = keys[p];
  float d = 0.f, nrm[3] = {0.f, 0.f, 0.f}, c[3] = {0.f, 0.f, 0.f};
  int32_t fid = -1;
  if (key != MR_EMPTY_KEY) {
    const uint32_t face = (uint32_t)key;
    if ((long long)face < P.n) {
      fid = (int32_t)face;
      d = mr_key_depth(key);
      mr_resolve_pixel(rec, faces, vertices, COLORS ? colors : nullptr, NORMALS == 2 ? vnormals : nullptr, P.camera_sign, face, col,
                       row, NORMALS != 0, nrm, c);
    } else {
      __hip_atomic_fetch_or((unsigned long long*)&state[MR_STATE_STATUS], (unsigned long long)MESH_ST_BAD_INDEX, MR_RLX);
    }
  }
  depth[p] = d;
  face_out[p] = fid;
  if (NORMALS) {
#pragma unroll
    for (int a = 0; a < 3; ++a) normal[a * N + p] = nrm[a];
  }
  if (COLORS) {
#pragma unroll
    for (int a = 0; a < 3; ++a) rgb[a * N + p] = c[a];
  }
}

}  // namespace sfgs

using namespace sfgs;

namespace {

struct MrScratch {
  unsigned long long *list_count, *count_lines;   // [2] (+ padding), [MR_COUNT_LINES][MR_COUNT_STRIDE]: cleared by every call
  size_t zero_bytes;
  MrVertex* rec; unsigned long long* keys; uint32_t *list_large, *list_huge; size_t total;
};

MrScratch mr_scratch(void* base, long long m, long long n, long long pixels) {
  MrScratch s;
  char* p = (char*)base;
  size_t off = 0;
  s.list_count = (unsigned long long*)(p + off); off += 256;
  s.count_lines = (unsigned long long*)(p + off); off += (size_t)MR_COUNT_LINES * MR_COUNT_STRIDE * 8;
  s.zero_bytes = off;
  s.rec = (MrVertex*)(p + off); off += align_up((size_t)m * sizeof(MrVertex), 256);
  s.keys = (unsigned long long*)(p + off); off += align_up((size_t)pixels * 8, 256);
  s.list_large = (uint32_t*)(p + off); off += align_up((size_t)n * 4, 256);
  s.list_huge = (uint32_t*)(p + off); off += align_up((size_t)n * 4, 256);
  s.total = off;
  return s;
}

int mr_check_sizes(const char* what, int64_t m, int64_t n, int32_t H, int32_t W) {
  SFGS_REQUIRE(n >= 0 && n <= MESH_MAX_TRIANGLES, SFGS_E_ARG, "%s: n = %lld outside 0 ... 2^29", what, (long long)n);
  SFGS_REQUIRE(m >= 0 && m <= MESH_MAX_VERTICES, SFGS_E_ARG, "%s: m = %lld outside 0 ... 2^31 - 1", what, (long long)m);
  SFGS_REQUIRE(m > 0 || n == 0, SFGS_E_ARG, "%s: %lld faces over no vertex", what, (long long)n);
  SFGS_REQUIRE(H > 0 && W > 0, SFGS_E_ARG, "%s: H %d, W %d", what, H, W);
  SFGS_REQUIRE((long long)H * W <= (1ll << 30), SFGS_E_ARG, "%s: H * W must not exceed 2^30, got %d x %d", what, H, W);
  return SFGS_OK;
}

template <int NORMALS>
void mr_resolve_launch(dim3 grid, hipStream_t stream, const MrParams& P, const MrScratch& s, const SfgsMeshRender* a) {
  if (a->colors)
    hipLaunchKernelGGL((mr_resolve_kernel<NORMALS, true>), grid, dim3(MR_THREADS), 0, stream, P, (const MrVertex*)s.rec, a->faces,
                       a->vertices, a->colors, a->vertex_normals, (const unsigned long long*)s.keys, a->depth, a->face, a->normal,
                       a->rgb, (const unsigned long long*)s.count_lines, a->state);
  else
    hipLaunchKernelGGL((mr_resolve_kernel<NORMALS, false>), grid, dim3(MR_THREADS), 0, stream, P, (const MrVertex*)s.rec, a->faces,
                       a->vertices, a->colors, a->vertex_normals, (const unsigned long long*)s.keys, a->depth, a->face, a->normal,
                       a->rgb, (const unsigned long long*)s.count_lines, a->state);
}

}  // namespace

extern "C" size_t sfgs_mesh_render_scratch_bytes(int64_t m, int64_t n, int32_t H, int32_t W) {
  if (mr_check_sizes("sfgs_mesh_render_scratch_bytes", m, n, H, W)) return 0;
  return mr_scratch(nullptr, m, n, (long long)H * W).total;
}

extern "C" int sfgs_mesh_render(const SfgsMeshRender* a, void* scratch, size_t scratch_bytes, void* stream_) {
  SFGS_REQUIRE(a, SFGS_E_ARG, "NULL SfgsMeshRender");
  SFGS_REQUIRE(a->struct_size == sizeof(SfgsMeshRender), SFGS_E_ARG, "SfgsMeshRender.struct_size %u, expected %zu", a->struct_size,
               sizeof(SfgsMeshRender));
  if (const int rc = mr_check_sizes("sfgs_mesh_render", a->m, a->n, a->H, a->W)) return rc;
  for (int k = 0; k < 9; ++k) SFGS_REQUIRE(fabs(a->M[k]) < INFINITY, SFGS_E_ARG, "SfgsMeshRender.M[%d] %g: finite", k, a->M[k]);
  for (int k = 0; k < 3; ++k) SFGS_REQUIRE(fabs(a->c[k]) < INFINITY, SFGS_E_ARG, "SfgsMeshRender.c[%d] %g: finite", k, a->c[k]);
  SFGS_REQUIRE(fabs(a->cx_pix) < INFINITY && fabs(a->cy_pix) < INFINITY, SFGS_E_ARG, "SfgsMeshRender: principal point %g, %g: finite",
               a->cx_pix, a->cy_pix);
  SFGS_REQUIRE(a->focal_x != 0.0 && a->focal_y != 0.0 && fabs(a->focal_x) < INFINITY && fabs(a->focal_y) < INFINITY, SFGS_E_ARG,
               "SfgsMeshRender: focal %g, %g: finite and non-zero", a->focal_x, a->focal_y);
  SFGS_REQUIRE(a->near >= 0.0 && a->near < INFINITY, SFGS_E_ARG, "SfgsMeshRender.near %g: finite and >= 0", a->near);
  SFGS_REQUIRE(a->far > a->near, SFGS_E_ARG, "SfgsMeshRender.far %g: above near %g", a->far, a->near);      // NaN fails
  SFGS_REQUIRE(a->cull == 0 || a->cull == 1, SFGS_E_ARG, "SfgsMeshRender.cull %d: 0 (none) or 1 (back)", a->cull);
  SFGS_REQUIRE(a->small_max >= -1 && a->small_max <= (1ll << 30), SFGS_E_ARG, "SfgsMeshRender.small_max %lld: -1 (default) ... 2^30",
               (long long)a->small_max);
  SFGS_REQUIRE(a->m == 0 || a->vertices, SFGS_E_ARG, "SfgsMeshRender: NULL vertices");
  SFGS_REQUIRE(a->n == 0 || a->faces, SFGS_E_ARG, "SfgsMeshRender: NULL faces");
  SFGS_REQUIRE(a->depth && a->face && a->state, SFGS_E_ARG, "SfgsMeshRender: NULL depth, face or state");
  SFGS_REQUIRE((a->colors == nullptr) == (a->rgb == nullptr), SFGS_E_ARG, "SfgsMeshRender: colors and rgb come together");
  SFGS_REQUIRE(!a->vertex_normals || a->normal, SFGS_E_ARG, "SfgsMeshRender: vertex_normals without a normal output");
  SFGS_REQUIRE(scratch, SFGS_E_ARG, "sfgs_mesh_render: NULL scratch");
  const long long pixels = (long long)a->H * a->W;
  const MrScratch s = mr_scratch(scratch, a->m, a->n, pixels);
  SFGS_REQUIRE(scratch_bytes >= s.total, SFGS_E_ARG, "mesh render scratch too small: %zu < %zu", scratch_bytes, s.total);
  hipStream_t stream = (hipStream_t)stream_;
  MrParams P;
  for (int k = 0; k < 9; ++k) P.cam.M[k] = a->M[k];
  for (int k = 0; k < 3; ++k) { P.cam.c[k] = a->c[k]; P.cam.origin[k] = 0.0; }
  P.cam.cx_pix = a->cx_pix; P.cam.cy_pix = a->cy_pix; P.cam.focal_x = a->focal_x; P.cam.focal_y = a->focal_y;
  P.near = a->near; P.far = a->far; P.H = a->H; P.W = a->W;
  P.camera_sign = mr_camera_sign(P.cam);
  P.cull = a->cull;
  P.m = a->m; P.n = a->n;
  P.small_max = a->small_max < 0 ? MR_SMALL_MAX_DEFAULT : a->small_max;
  SFGS_CHECK_HIP(hipMemsetAsync(a->state, 0, 8 * sizeof(long long), stream));
  SFGS_CHECK_HIP(hipMemsetAsync(s.list_count, 0, s.zero_bytes, stream));
  SFGS_CHECK_HIP(hipMemsetAsync(s.keys, 0xff, (size_t)pixels * 8, stream));
  if (a->n > 0) {
    hipLaunchKernelGGL(mr_project_kernel, dim3((unsigned)((a->m + MR_THREADS - 1) / MR_THREADS)), dim3(MR_THREADS), 0, stream, P,
                       a->vertices, s.rec);
    SFGS_POST_LAUNCH("mr_project", stream, 0);
    hipLaunchKernelGGL(mr_face_kernel, dim3((unsigned)((a->n + MR_THREADS - 1) / MR_THREADS)), dim3(MR_THREADS), 0, stream, P,
                       (const MrVertex*)s.rec, a->faces, s.keys, s.list_large, s.list_huge, s.list_count, s.count_lines, a->state);
    SFGS_POST_LAUNCH("mr_face", stream, 0);
    if (P.small_max < pixels) {                           // otherwise no box exceeds small_max: the lists stay empty
      hipLaunchKernelGGL(mr_large_kernel, dim3(MR_LARGE_BLOCKS), dim3(MR_THREADS), 0, stream, P, (const MrVertex*)s.rec, a->faces, s.keys,
                         (const uint32_t*)s.list_large, (const uint32_t*)s.list_huge, (const unsigned long long*)s.list_count, a->state);
      SFGS_POST_LAUNCH("mr_large", stream, 0);
    }
  }
  // resolve's workgroups: at most 2^30 / 256 + a partial row and column of them, far below 2^31 (H W <= 2^30 was checked)
  const dim3 grid((unsigned)((a->W + MR_TILE - 1) / MR_TILE) * (unsigned)((a->H + MR_TILE - 1) / MR_TILE));
  if (!a->normal) mr_resolve_launch<0>(grid, stream, P, s, a);
  else if (!a->vertex_normals) mr_resolve_launch<1>(grid, stream, P, s, a);
  else mr_resolve_launch<2>(grid, stream, P, s, a);
  SFGS_POST_LAUNCH("mr_resolve", stream, 0);
  return SFGS_OK;
}
