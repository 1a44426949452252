// tsdf.hip -- depth views -> a truncated signed distance volume -> a triangle soup, or views ray-cast from it: the surface the other geometry products
// (geometry.hip: a 2.5-D height grid; pointcloud.hip: unconnected points) do not give. The reference has no mesh step. The
// per-voxel update and the per-cell marching-tetrahedra triangulation are tsdf_math.h's (built for the host too, by
// tests/host_check/tsdf_check.cpp); include/sfgs.h states both sequences in words and tests/tsdf_np.py in numpy; this file is held
// to that restatement bit for bit.
//   tsdf_integrate_kernel, ONE launch for a batch of <= 256 views: a thread owns a voxel, keeps (D, W, rgb) in registers and
//     walks the views in ascending order (geo_project -> nearest pixel, range-checked on the doubles -> its depth, if used ->
//     sdf -> running mean). The view loop is uniform across the wave: the record of view j -- pointers, size, camera -- comes
//     from the device table by scalar loads, as in cons_check_kernel. The voxel is stored only if some view updated it.
//     No atomics of any kind, no shared words, no barrier.
//     Layout: a workgroup is a brick of 8 x 8 x 4 voxels, a wave an 8 x 8 slab of it, so that the 64 gathers of a wave fall into
//     a compact window of the view. The run of 256 voxels along x takes 7.36 ms where the brick takes 2.49 ms, on 24 views of
//     1024 x 1024 into 512 x 512 x 128 voxels (tools/variants/tsdf_run_x.patch, profiles/r22_tsdf_ab.txt).
//   extraction, three launches modelled on pc_count / pc_scan / pc_scatter (no kernel waits for another workgroup):
//     1. tsdf_count_kernel  a workgroup owns TSDF_THREADS consecutive cells and writes how many triangles they hold (0 ... 12 each);
//     2. scan_sums_kernel   (scan.h) ONE workgroup scans the counts exclusively, 1024 at a time with a carry, and leaves the total in *state;
//     3. tsdf_emit_kernel   recomputes the cells, ranks their triangles inside the workgroup and writes the workgroup's run.
//     The soup is ordered by cell, tetrahedron, triangle. A row at or beyond `capacity` is not written; the state counts it.
//   ray-casting, ONE launch per view (tsdf_math.h: tsdf_ray_pixel; tests/tsdf_raycast_np.py in numpy, held to it byte for byte):
//     tsdf_raycast_kernel<COLORS, NORMALS, SKIP>  a thread owns a pixel: its ray is cut to the box of voxel centres and marched on
//       a lattice of depths; a sample gathers the eight voxels (and weights) of its cell into registers, static indices only; the
//       hit is the first valid sample < 0 behind a valid sample >= 0. Gradient and colour of the two bracketing samples are
//       gathered after the march, not in it. Rays diverge in length: a wave is an 8 x 8 tile of pixels (a workgroup 16 x 16), so
//       its rays stay together and its gathers fall into a compact part of the volume. No LDS, no atomics, no barrier.
//     tsdf_skip_kernel  the empty-space table: a workgroup per brick of 8^3 cells ORs `observed and inside` over the brick's
//       footprint of at most 9^3 voxels (__syncthreads_or) and stores one byte. With SKIP the march does not evaluate samples in
//       bricks whose byte is 0 and jumps over runs of them; the outputs are the same bytes.
// Every index is range-checked before it is used: a voxel against the volume before its load and store, a pixel against its view's
// H x W (on the doubles) before its load, a cell against the cell grid before its eight corners, a row against capacity; in the
// ray-cast a cell comes out of a clamp to [0, n - 2] on the double, a brick is checked against the table's dims before its load,
// a pixel against H x W before any load or store.
// No profiler ids.
#include "sfgs_internal.h"
#include "scan.h"
#include "tsdf_math.h"

#include <math.h>

namespace sfgs {

constexpr int TSDF_THREADS = 256;
constexpr int TSDF_WAVES = TSDF_THREADS / 64;
constexpr int TSDF_BRICK_X = 8, TSDF_BRICK_Y = 8, TSDF_BRICK_Z = 4;     // TSDF_THREADS voxels; a wave is one z-slab of it
static_assert(TSDF_BRICK_X * TSDF_BRICK_Y == 64 && TSDF_BRICK_X * TSDF_BRICK_Y * TSDF_BRICK_Z == TSDF_THREADS, "a wave is a slab");

// the table's record as the kernel reads it: the layout of SfgsTsdfView (checked below)
struct TsdfView {
  const float* depth;
  const unsigned char* mask;
  const float* image;
  int H, W;
  double M[9], c[3];
  double cx_pix, cy_pix, focal_x, focal_y;
};
static_assert(sizeof(TsdfView) == sizeof(SfgsTsdfView), "TsdfView is SfgsTsdfView");
static_assert(offsetof(TsdfView, image) == offsetof(SfgsTsdfView, image) && offsetof(TsdfView, H) == offsetof(SfgsTsdfView, H) &&
              offsetof(TsdfView, M) == offsetof(SfgsTsdfView, M) && offsetof(TsdfView, c) == offsetof(SfgsTsdfView, c) &&
              offsetof(TsdfView, cx_pix) == offsetof(SfgsTsdfView, cx_pix) && offsetof(TsdfView, focal_y) == offsetof(SfgsTsdfView, focal_y),
              "TsdfView is SfgsTsdfView");

struct TsdfGrid {
  int nx, ny, nz;
  double origin[3], voxel_size, trunc, max_weight;
};

__device__ __forceinline__ GeoCamera tsdf_camera(const TsdfView& r) {
  GeoCamera g;
#pragma unroll
  for (int k = 0; k < 9; ++k) g.M[k] = r.M[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) { g.c[k] = r.c[k]; g.origin[k] = 0.0; }
  g.cx_pix = r.cx_pix; g.cy_pix = r.cy_pix; g.focal_x = r.focal_x; g.focal_y = r.focal_y;
  return g;
}

template <bool COLORS>
__global__ void __launch_bounds__(TSDF_THREADS)
tsdf_integrate_kernel(const TsdfView* __restrict__ table, int V, TsdfGrid g, float* __restrict__ tsdf, float* __restrict__ weight,
                      float* __restrict__ rgb) {
  const unsigned bricks_x = (unsigned)((g.nx + TSDF_BRICK_X - 1) / TSDF_BRICK_X), bricks_y = (unsigned)((g.ny + TSDF_BRICK_Y - 1) / TSDF_BRICK_Y);
  const unsigned bz = blockIdx.x / (bricks_x * bricks_y), rest = blockIdx.x - bz * (bricks_x * bricks_y);
  const unsigned by = rest / bricks_x, bx = rest - by * bricks_x;
  const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const int i = (int)(bx * TSDF_BRICK_X + (lane & 7u)), j = (int)(by * TSDF_BRICK_Y + (lane >> 3)), k = (int)(bz * TSDF_BRICK_Z + wave);
  if (i >= g.nx || j >= g.ny || k >= g.nz) return;   // no barrier follows
  const long long nvox = (long long)g.nx * g.ny * g.nz;
  const long long p = ((long long)k * g.ny + j) * g.nx + i;
  const double centre[3] = {tsdf_centre(g.origin[0], i, g.voxel_size), tsdf_centre(g.origin[1], j, g.voxel_size),
                            tsdf_centre(g.origin[2], k, g.voxel_size)};
  float D = tsdf[p], Wt = weight[p], col[3] = {0.f, 0.f, 0.f};
  if (COLORS) {
#pragma unroll
    for (int c = 0; c < 3; ++c) col[c] = rgb[(long long)c * nvox + p];
  }
  bool touched = false;
  for (int v = 0; v < V; ++v) {                      // uniform: v and the record are the same in every lane
    const TsdfView& S = table[v];
    const GeoCamera cam = tsdf_camera(S);
    touched |= tsdf_update<COLORS>(cam, S.H, S.W, S.depth, S.mask, S.image, centre, g.trunc, g.max_weight, &D, &Wt, col) == TSDF_UPDATED;
  }
  if (!touched) return;
  tsdf[p] = D;
  weight[p] = Wt;
  if (COLORS) {
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb[(long long)c * nvox + p] = col[c];
  }
}

// ---- extraction ------------------------------------------------------------------------------------------------------------------
struct TsdfCells {
  int nx, ny, nz;            // of the VOLUME; the cell grid is one smaller along each axis
  long long ncells;
};

// Cell `cell` < ncells -> its position and its eight corner values (and colours); false when a corner weight is not > 0.
template <bool COLORS>
__device__ __forceinline__ bool tsdf_load_cell(const TsdfCells& g, long long cell, const float* __restrict__ tsdf,
                                               const float* __restrict__ weight, const float* __restrict__ rgb, int* x, int* y, int* z,
                                               float (&val)[8], float (&col)[3][8]) {
  const int cx = g.nx - 1, cy = g.ny - 1;
  const long long row = cell / cx;
  *x = (int)(cell - row * cx);
  *z = (int)(row / cy);
  *y = (int)(row - (long long)*z * cy);
  const long long base = ((long long)*z * g.ny + *y) * g.nx + *x;          // *x + 1 < nx, *y + 1 < ny, *z + 1 < nz
  const long long plane = (long long)g.nx * g.ny;
  bool used = true;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const long long q = base + (k & 1) + (long long)((k >> 1) & 1) * g.nx + (long long)((k >> 2) & 1) * plane;
    used = used && weight[q] > 0.f;
    val[k] = tsdf[q];
  }
  if (COLORS && used) {
    const long long nvox = plane * g.nz;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int k = 0; k < 8; ++k)
        col[c][k] = rgb[c * nvox + base + (k & 1) + (long long)((k >> 1) & 1) * g.nx + (long long)((k >> 2) & 1) * plane];
  }
  return used;
}

__global__ void __launch_bounds__(TSDF_THREADS)
tsdf_count_kernel(TsdfCells g, const float* __restrict__ tsdf, const float* __restrict__ weight, unsigned long long* __restrict__ blk) {
  __shared__ unsigned wave_n[TSDF_WAVES];
  const long long cell = (long long)blockIdx.x * TSDF_THREADS + threadIdx.x;
  unsigned n = 0;
  if (cell < g.ncells) {
    int x, y, z;
    float val[8], col[3][8];
    if (tsdf_load_cell<false>(g, cell, tsdf, weight, nullptr, &x, &y, &z, val, col)) n = (unsigned)tsdf_cell_count(val);
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) n += __shfl_down(n, d);
  if (lane_id() == 0) wave_n[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned total = 0;
#pragma unroll
    for (int w = 0; w < TSDF_WAVES; ++w) total += wave_n[w];
    blk[blockIdx.x] = total;
  }
}

template <bool COLORS>
__global__ void __launch_bounds__(TSDF_THREADS)
tsdf_emit_kernel(TsdfCells g, TsdfMeshFrame f, const float* __restrict__ tsdf, const float* __restrict__ weight,
                 const float* __restrict__ rgb, const unsigned long long* __restrict__ blk, float* __restrict__ vertices,
                 float* __restrict__ colors, long long capacity) {
  __shared__ unsigned smem[TSDF_WAVES + 1];
  const long long cell = (long long)blockIdx.x * TSDF_THREADS + threadIdx.x;
  int x = 0, y = 0, z = 0;
  float val[8], col[3][8];
  const bool used = cell < g.ncells && tsdf_load_cell<COLORS>(g, cell, tsdf, weight, rgb, &x, &y, &z, val, col);
  const unsigned n = used ? (unsigned)tsdf_cell_count(val) : 0u;
  unsigned total;
  const unsigned before = block_excl_scan_u32<TSDF_THREADS>(n, &total, smem);      // every thread reaches the barriers
  if (n == 0) return;
  const unsigned long long first = blk[blockIdx.x] + before;
  if (first >= (unsigned long long)capacity) return;
  tsdf_cell_emit<COLORS>(f, val, col, x, y, z, vertices, colors, (long long)first, capacity);
}

// ---- ray-casting -----------------------------------------------------------------------------------------------------------------
constexpr int TSDF_RAY_TILE = 16;                    // a workgroup is 16 x 16 pixels, a wave an 8 x 8 quarter of it
static_assert(TSDF_RAY_TILE * TSDF_RAY_TILE == TSDF_THREADS && TSDF_WAVES == 4, "four 8 x 8 waves");

// One workgroup per brick of 8^3 cells: its byte is non-zero when a voxel of the footprint (at most 9^3) is observed and inside.
__global__ void __launch_bounds__(TSDF_THREADS)
tsdf_skip_kernel(TsdfRayGrid g, const float* __restrict__ tsdf, const float* __restrict__ weight, unsigned char* __restrict__ skip) {
  const unsigned per_z = (unsigned)(g.bx * g.by);
  const unsigned bz = blockIdx.x / per_z, rest = blockIdx.x - bz * per_z;
  const unsigned by = rest / (unsigned)g.bx, bx = rest - by * (unsigned)g.bx;
  if (bz >= (unsigned)g.bz) return;                  // the whole workgroup: no thread reaches the barrier
  const int lo[3] = {(int)bx * TSDF_SKIP_BRICK, (int)by * TSDF_SKIP_BRICK, (int)bz * TSDF_SKIP_BRICK};
  const int n[3] = {g.nx, g.ny, g.nz};
  int hi[3];                                         // the footprint's last voxel per axis
#pragma unroll
  for (int a = 0; a < 3; ++a) hi[a] = lo[a] + TSDF_SKIP_BRICK < n[a] - 1 ? lo[a] + TSDF_SKIP_BRICK : n[a] - 1;
  constexpr int E = TSDF_SKIP_BRICK + 1;             // a full footprint is E^3 voxels: constant divisors, a partial one skips
  int any = 0;
  for (int t = (int)threadIdx.x; t < E * E * E; t += TSDF_THREADS) {
    const int tz = t / (E * E), r = t - tz * (E * E);
    const int ty = r / E, tx = r - ty * E;
    const int x = lo[0] + tx, y = lo[1] + ty, z = lo[2] + tz;
    if (x <= hi[0] && y <= hi[1] && z <= hi[2]) {       // hi < n: inside the volume
      const long long p = ((long long)z * g.ny + y) * g.nx + x;
      any |= tsdf_skip_flag(weight[p], tsdf[p]) ? 1 : 0;
    }
  }
  any = __syncthreads_or(any);
  if (threadIdx.x == 0) skip[blockIdx.x] = any ? 1 : 0;
}

// One thread per pixel; tiles are numbered row by row in blockIdx.x. The rays of a wave leave an 8 x 8 patch of the image, so
// their gathers stay in a compact part of the volume. Grid and camera are kernel arguments: uniform, read by scalar loads.
template <bool COLORS, bool NORMALS, bool SKIP>
__global__ void __launch_bounds__(TSDF_THREADS)
tsdf_raycast_kernel(TsdfRayGrid g, TsdfRayCamera cam, int H, int W, const float* __restrict__ tsdf, const float* __restrict__ weight,
                    const float* __restrict__ rgb, const unsigned char* __restrict__ skip, float* __restrict__ depth,
                    float* __restrict__ normal, float* __restrict__ colour) {
  const unsigned tiles_x = (unsigned)((W + TSDF_RAY_TILE - 1) / TSDF_RAY_TILE);
  const unsigned tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
  const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const int col = (int)(tile_x * TSDF_RAY_TILE + (wave & 1u) * 8u + (lane & 7u));
  const int row = (int)(tile_y * TSDF_RAY_TILE + (wave >> 1) * 8u + (lane >> 3));
  if (row >= H || col >= W) return;                  // before any load; no barrier follows
  float dep, nrm[3], rgb_out[3];
  tsdf_ray_pixel<COLORS, NORMALS, SKIP>(g, cam, row, col, tsdf, weight, rgb, skip, &dep, nrm, rgb_out, nullptr);
  const long long P = (long long)H * W, p = (long long)row * W + col;
  depth[p] = dep;
  if (NORMALS) {
#pragma unroll
    for (int c = 0; c < 3; ++c) normal[c * P + p] = nrm[c];
  }
  if (COLORS) {
#pragma unroll
    for (int c = 0; c < 3; ++c) colour[c * P + p] = rgb_out[c];
  }
}

}  // namespace sfgs

using namespace sfgs;

namespace {

// Every refusal of this file is SFGS_E_ARG: the caller made the call wrong, nothing was launched.
int tsdf_check_dims(const char* what, int32_t nx, int32_t ny, int32_t nz) {
  SFGS_REQUIRE(nx > 0 && ny > 0 && nz > 0, SFGS_E_ARG, "%s: dims %d x %d x %d", what, nx, ny, nz);
  SFGS_REQUIRE((long long)nx * ny <= (1ll << 30) && (long long)nx * ny * nz <= (1ll << 30), SFGS_E_ARG,
               "%s: nx * ny * nz must not exceed 2^30, got %d x %d x %d", what, nx, ny, nz);
  return SFGS_OK;
}

int tsdf_check_volume(const SfgsTsdfVolume* v) {
  SFGS_REQUIRE(v, SFGS_E_ARG, "NULL SfgsTsdfVolume");
  SFGS_REQUIRE(v->struct_size == sizeof(SfgsTsdfVolume), SFGS_E_ARG, "SfgsTsdfVolume.struct_size %u, expected %zu", v->struct_size,
               sizeof(SfgsTsdfVolume));
  if (const int rc = tsdf_check_dims("SfgsTsdfVolume", v->nx, v->ny, v->nz)) return rc;
  SFGS_REQUIRE(v->voxel_size > 0.0 && v->voxel_size < INFINITY, SFGS_E_ARG, "SfgsTsdfVolume.voxel_size %g: finite and > 0", v->voxel_size);
  SFGS_REQUIRE(v->trunc > 0.0 && v->trunc < INFINITY, SFGS_E_ARG, "SfgsTsdfVolume.trunc %g: finite and > 0", v->trunc);
  SFGS_REQUIRE(v->max_weight >= 1.0, SFGS_E_ARG, "SfgsTsdfVolume.max_weight %g: >= 1", v->max_weight);
  for (int a = 0; a < 3; ++a)
    SFGS_REQUIRE(fabs(v->origin[a]) < INFINITY, SFGS_E_ARG, "SfgsTsdfVolume.origin[%d] %g: finite", a, v->origin[a]);
  SFGS_REQUIRE(v->tsdf && v->weight, SFGS_E_ARG, "SfgsTsdfVolume: NULL tsdf or weight");
  return SFGS_OK;
}

inline long long tsdf_cells(int32_t nx, int32_t ny, int32_t nz) { return (long long)(nx - 1) * (ny - 1) * (nz - 1); }
inline long long tsdf_cell_blocks(long long ncells) { return (ncells + TSDF_THREADS - 1) / TSDF_THREADS; }
size_t tsdf_scratch_bytes(int32_t nx, int32_t ny, int32_t nz) {
  return align_up((size_t)(tsdf_cell_blocks(tsdf_cells(nx, ny, nz)) + 1) * 8, 256);
}

}  // namespace

extern "C" int sfgs_tsdf_table_check(const SfgsTsdfView* views, int32_t V, int32_t with_images) {
  SFGS_REQUIRE(views, SFGS_E_ARG, "NULL SfgsTsdfView table");
  SFGS_REQUIRE(V >= 1 && V <= TSDF_MAX_VIEWS, SFGS_E_ARG, "tsdf: %d views, 1 ... %d", V, TSDF_MAX_VIEWS);
  for (int k = 0; k < V; ++k) {
    const SfgsTsdfView& r = views[k];
    SFGS_REQUIRE(r.H > 0 && r.W > 0, SFGS_E_ARG, "SfgsTsdfView %d: H %d, W %d", k, r.H, r.W);
    SFGS_REQUIRE((long long)r.H * r.W <= (1ll << 30), SFGS_E_ARG, "SfgsTsdfView %d: H * W must not exceed 2^30, got %d x %d", k, r.H, r.W);
    SFGS_REQUIRE(r.depth, SFGS_E_ARG, "SfgsTsdfView %d: NULL depth", k);
    SFGS_REQUIRE(r.focal_x != 0.0 && r.focal_y != 0.0, SFGS_E_ARG, "SfgsTsdfView %d: focal %g, %g", k, r.focal_x, r.focal_y);
    SFGS_REQUIRE((r.image != nullptr) == (with_images != 0), SFGS_E_ARG,
                 "SfgsTsdfView %d: an image is given exactly when the volume keeps colours", k);
  }
  return SFGS_OK;
}

extern "C" int sfgs_tsdf_integrate(const SfgsTsdfVolume* vol, const void* table, int32_t V, void* stream_) {
  if (const int rc = tsdf_check_volume(vol)) return rc;
  SFGS_REQUIRE(V >= 1 && V <= TSDF_MAX_VIEWS, SFGS_E_ARG, "sfgs_tsdf_integrate: %d views, 1 ... %d", V, TSDF_MAX_VIEWS);
  SFGS_REQUIRE(table, SFGS_E_ARG, "sfgs_tsdf_integrate: NULL table");
  TsdfGrid g;
  g.nx = vol->nx; g.ny = vol->ny; g.nz = vol->nz;
  for (int a = 0; a < 3; ++a) g.origin[a] = vol->origin[a];
  g.voxel_size = vol->voxel_size; g.trunc = vol->trunc; g.max_weight = vol->max_weight;
  hipStream_t stream = (hipStream_t)stream_;
  const long long bricks = (long long)((g.nx + TSDF_BRICK_X - 1) / TSDF_BRICK_X) * ((g.ny + TSDF_BRICK_Y - 1) / TSDF_BRICK_Y) *
                           ((g.nz + TSDF_BRICK_Z - 1) / TSDF_BRICK_Z);                  // <= 2^30 / 4 + the partial ones
  SFGS_REQUIRE(bricks <= 0x7fffffffll, SFGS_E_ARG, "sfgs_tsdf_integrate: %lld workgroups", bricks);
  const dim3 grid((unsigned)bricks), block(TSDF_THREADS);
  if (vol->rgb)
    hipLaunchKernelGGL(tsdf_integrate_kernel<true>, grid, block, 0, stream, (const TsdfView*)table, V, g, vol->tsdf, vol->weight, vol->rgb);
  else
    hipLaunchKernelGGL(tsdf_integrate_kernel<false>, grid, block, 0, stream, (const TsdfView*)table, V, g, vol->tsdf, vol->weight, vol->rgb);
  SFGS_POST_LAUNCH("tsdf_integrate", stream, 0);
  return SFGS_OK;
}

extern "C" size_t sfgs_tsdf_scratch_bytes(int32_t nx, int32_t ny, int32_t nz) {
  if (tsdf_check_dims("sfgs_tsdf_scratch_bytes", nx, ny, nz)) return 0;
  return tsdf_scratch_bytes(nx, ny, nz);
}

extern "C" int sfgs_tsdf_extract(const SfgsTsdfVolume* vol, float* vertices, float* colors, int64_t capacity, unsigned long long* state,
                                 void* scratch, size_t scratch_bytes, void* stream_) {
  if (const int rc = tsdf_check_volume(vol)) return rc;
  SFGS_REQUIRE(capacity >= 0, SFGS_E_ARG, "sfgs_tsdf_extract: capacity %lld", (long long)capacity);
  SFGS_REQUIRE(vertices && state && scratch, SFGS_E_ARG, "NULL argument");
  SFGS_REQUIRE((vol->rgb == nullptr) == (colors == nullptr), SFGS_E_ARG, "sfgs_tsdf_extract: SfgsTsdfVolume.rgb and colors come together");
  const size_t need = tsdf_scratch_bytes(vol->nx, vol->ny, vol->nz);
  SFGS_REQUIRE(scratch_bytes >= need, SFGS_E_ARG, "tsdf scratch too small: %zu < %zu", scratch_bytes, need);
  TsdfCells g;
  g.nx = vol->nx; g.ny = vol->ny; g.nz = vol->nz;
  g.ncells = tsdf_cells(vol->nx, vol->ny, vol->nz);
  TsdfMeshFrame f;
  for (int a = 0; a < 3; ++a) f.origin[a] = (float)vol->origin[a];
  f.voxel_size = (float)vol->voxel_size;
  hipStream_t stream = (hipStream_t)stream_;
  const long long nblk = tsdf_cell_blocks(g.ncells);       // 0 for a volume one voxel thick: only the scan runs, and writes 0
  unsigned long long* blk = (unsigned long long*)scratch;
  const dim3 grid((unsigned)nblk), block(TSDF_THREADS);
  if (nblk > 0) {
    hipLaunchKernelGGL(tsdf_count_kernel, grid, block, 0, stream, g, (const float*)vol->tsdf, (const float*)vol->weight, blk);
    SFGS_POST_LAUNCH("tsdf_count", stream, 0);
  }
  // blk[b]: count -> first row of workgroup b; *state = the total (what was there before is not read)
  hipLaunchKernelGGL(scan_sums_kernel<unsigned long long>, dim3(1), dim3(SCAN_TOP_THREADS), 0, stream, blk, nblk, 1,
                     (const unsigned long long*)nullptr, state);
  SFGS_POST_LAUNCH("tsdf_scan", stream, 0);
  if (nblk > 0) {
    if (colors)
      hipLaunchKernelGGL(tsdf_emit_kernel<true>, grid, block, 0, stream, g, f, (const float*)vol->tsdf, (const float*)vol->weight,
                         (const float*)vol->rgb, (const unsigned long long*)blk, vertices, colors, (long long)capacity);
    else
      hipLaunchKernelGGL(tsdf_emit_kernel<false>, grid, block, 0, stream, g, f, (const float*)vol->tsdf, (const float*)vol->weight,
                         (const float*)vol->rgb, (const unsigned long long*)blk, vertices, colors, (long long)capacity);
    SFGS_POST_LAUNCH("tsdf_emit", stream, 0);
  }
  return SFGS_OK;
}

// ---- ray-casting -----------------------------------------------------------------------------------------------------------------
namespace {

TsdfRayGrid tsdf_ray_grid(const SfgsTsdfVolume* vol) {
  TsdfRayGrid g;
  g.nx = vol->nx; g.ny = vol->ny; g.nz = vol->nz;
  g.bx = tsdf_skip_bricks(vol->nx); g.by = tsdf_skip_bricks(vol->ny); g.bz = tsdf_skip_bricks(vol->nz);
  for (int a = 0; a < 3; ++a) g.origin[a] = vol->origin[a];
  g.voxel_size = vol->voxel_size;
  g.inv_voxel = 1.0 / vol->voxel_size;
  return g;
}

inline size_t tsdf_skip_table_bytes(int32_t nx, int32_t ny, int32_t nz) {
  return (size_t)tsdf_skip_bricks(nx) * (size_t)tsdf_skip_bricks(ny) * (size_t)tsdf_skip_bricks(nz);      // <= 2^30
}

inline bool tsdf_has_cells(const SfgsTsdfVolume* vol) { return vol->nx >= 2 && vol->ny >= 2 && vol->nz >= 2; }

template <bool COLORS, bool NORMALS, bool SKIP>
void tsdf_raycast_launch(dim3 grid, hipStream_t stream, const TsdfRayGrid& g, const TsdfRayCamera& cam, const SfgsTsdfVolume* vol,
                         const SfgsTsdfRay* ray, const unsigned char* skip) {
  hipLaunchKernelGGL((tsdf_raycast_kernel<COLORS, NORMALS, SKIP>), grid, dim3(TSDF_THREADS), 0, stream, g, cam, ray->H, ray->W,
                     (const float*)vol->tsdf, (const float*)vol->weight, (const float*)vol->rgb, skip, ray->depth, ray->normal, ray->rgb);
}

template <bool COLORS, bool NORMALS>
void tsdf_raycast_launch(dim3 grid, hipStream_t stream, const TsdfRayGrid& g, const TsdfRayCamera& cam, const SfgsTsdfVolume* vol,
                         const SfgsTsdfRay* ray, const unsigned char* skip) {
  if (skip) tsdf_raycast_launch<COLORS, NORMALS, true>(grid, stream, g, cam, vol, ray, skip);
  else tsdf_raycast_launch<COLORS, NORMALS, false>(grid, stream, g, cam, vol, ray, skip);
}

}  // namespace

extern "C" size_t sfgs_tsdf_skip_bytes(int32_t nx, int32_t ny, int32_t nz) {
  if (tsdf_check_dims("sfgs_tsdf_skip_bytes", nx, ny, nz)) return 0;
  return tsdf_skip_table_bytes(nx, ny, nz);
}

extern "C" int sfgs_tsdf_skip_build(const SfgsTsdfVolume* vol, void* skip, size_t bytes, void* stream_) {
  if (const int rc = tsdf_check_volume(vol)) return rc;
  SFGS_REQUIRE(skip, SFGS_E_ARG, "sfgs_tsdf_skip_build: NULL table");
  const size_t need = tsdf_skip_table_bytes(vol->nx, vol->ny, vol->nz);
  SFGS_REQUIRE(bytes >= need, SFGS_E_ARG, "tsdf skip table too small: %zu < %zu", bytes, need);
  hipStream_t stream = (hipStream_t)stream_;
  if (!tsdf_has_cells(vol)) {                              // no cell, no ray-cast kernel will read the table: one zero byte
    SFGS_CHECK_HIP(hipMemsetAsync(skip, 0, need, stream));
    return SFGS_OK;
  }
  const TsdfRayGrid g = tsdf_ray_grid(vol);
  hipLaunchKernelGGL(tsdf_skip_kernel, dim3((unsigned)need), dim3(TSDF_THREADS), 0, stream, g, (const float*)vol->tsdf,
                     (const float*)vol->weight, (unsigned char*)skip);
  SFGS_POST_LAUNCH("tsdf_skip", stream, 0);
  return SFGS_OK;
}

extern "C" int sfgs_tsdf_raycast(const SfgsTsdfVolume* vol, const SfgsTsdfRay* ray, const void* skip, size_t skip_bytes, void* stream_) {
  if (const int rc = tsdf_check_volume(vol)) return rc;
  SFGS_REQUIRE(ray, SFGS_E_ARG, "NULL SfgsTsdfRay");
  SFGS_REQUIRE(ray->struct_size == sizeof(SfgsTsdfRay), SFGS_E_ARG, "SfgsTsdfRay.struct_size %u, expected %zu", ray->struct_size,
               sizeof(SfgsTsdfRay));
  SFGS_REQUIRE(ray->H > 0 && ray->W > 0, SFGS_E_ARG, "SfgsTsdfRay: H %d, W %d", ray->H, ray->W);
  SFGS_REQUIRE((long long)ray->H * ray->W <= (1ll << 30), SFGS_E_ARG, "SfgsTsdfRay: H * W must not exceed 2^30, got %d x %d", ray->H, ray->W);
  for (int k = 0; k < 9; ++k) SFGS_REQUIRE(fabs(ray->M[k]) < INFINITY, SFGS_E_ARG, "SfgsTsdfRay.M[%d] %g: finite", k, ray->M[k]);
  for (int k = 0; k < 3; ++k) SFGS_REQUIRE(fabs(ray->c[k]) < INFINITY, SFGS_E_ARG, "SfgsTsdfRay.c[%d] %g: finite", k, ray->c[k]);
  SFGS_REQUIRE(fabs(ray->cx_pix) < INFINITY && fabs(ray->cy_pix) < INFINITY, SFGS_E_ARG, "SfgsTsdfRay: principal point %g, %g: finite",
               ray->cx_pix, ray->cy_pix);
  SFGS_REQUIRE(ray->focal_x != 0.0 && ray->focal_y != 0.0 && fabs(ray->focal_x) < INFINITY && fabs(ray->focal_y) < INFINITY, SFGS_E_ARG,
               "SfgsTsdfRay: focal %g, %g: finite and non-zero", ray->focal_x, ray->focal_y);
  SFGS_REQUIRE(ray->near >= 0.0 && ray->near < INFINITY, SFGS_E_ARG, "SfgsTsdfRay.near %g: finite and >= 0", ray->near);
  SFGS_REQUIRE(ray->far > ray->near, SFGS_E_ARG, "SfgsTsdfRay.far %g: above near %g", ray->far, ray->near);      // NaN fails
  SFGS_REQUIRE(ray->step > 0.0 && ray->step < INFINITY, SFGS_E_ARG, "SfgsTsdfRay.step %g: finite and > 0", ray->step);
  const double ex = (vol->nx - 1) * vol->voxel_size, ey = (vol->ny - 1) * vol->voxel_size, ez = (vol->nz - 1) * vol->voxel_size;
  const double diagonal = sqrt(ex * ex + ey * ey + ez * ez);
  SFGS_REQUIRE(diagonal / ray->step <= (double)TSDF_RAY_MAX_SAMPLES, SFGS_E_ARG,
               "SfgsTsdfRay.step %g: the box diagonal %g holds more than 2^20 steps", ray->step, diagonal);
  SFGS_REQUIRE(ray->depth, SFGS_E_ARG, "SfgsTsdfRay: NULL depth");
  SFGS_REQUIRE((vol->rgb == nullptr) == (ray->rgb == nullptr), SFGS_E_ARG, "sfgs_tsdf_raycast: SfgsTsdfVolume.rgb and SfgsTsdfRay.rgb come together");
  const size_t need = tsdf_skip_table_bytes(vol->nx, vol->ny, vol->nz);
  SFGS_REQUIRE(!skip || skip_bytes >= need, SFGS_E_ARG, "tsdf skip table too small: %zu < %zu", skip_bytes, need);
  hipStream_t stream = (hipStream_t)stream_;
  const long long P = (long long)ray->H * ray->W;
  if (!tsdf_has_cells(vol)) {                              // every ray misses: the outputs of a miss, and no launch
    SFGS_CHECK_HIP(hipMemsetAsync(ray->depth, 0, (size_t)P * 4, stream));
    if (ray->normal) SFGS_CHECK_HIP(hipMemsetAsync(ray->normal, 0, (size_t)P * 12, stream));
    if (ray->rgb) SFGS_CHECK_HIP(hipMemsetAsync(ray->rgb, 0, (size_t)P * 12, stream));
    return SFGS_OK;
  }
  const TsdfRayGrid g = tsdf_ray_grid(vol);
  TsdfRayCamera cam;
  for (int k = 0; k < 9; ++k) cam.M[k] = ray->M[k];
  for (int k = 0; k < 3; ++k) cam.c[k] = ray->c[k];
  cam.cx_pix = ray->cx_pix; cam.cy_pix = ray->cy_pix; cam.focal_x = ray->focal_x; cam.focal_y = ray->focal_y;
  cam.near = ray->near; cam.far = ray->far; cam.step = ray->step;
  const long long tiles = (long long)((ray->W + TSDF_RAY_TILE - 1) / TSDF_RAY_TILE) * ((ray->H + TSDF_RAY_TILE - 1) / TSDF_RAY_TILE);
  SFGS_REQUIRE(tiles <= 0x7fffffffll, SFGS_E_ARG, "sfgs_tsdf_raycast: %lld workgroups", tiles);
  const dim3 grid((unsigned)tiles);
  const unsigned char* table = (const unsigned char*)skip;
  if (ray->rgb) {
    if (ray->normal) tsdf_raycast_launch<true, true>(grid, stream, g, cam, vol, ray, table);
    else tsdf_raycast_launch<true, false>(grid, stream, g, cam, vol, ray, table);
  } else {
    if (ray->normal) tsdf_raycast_launch<false, true>(grid, stream, g, cam, vol, ray, table);
    else tsdf_raycast_launch<false, false>(grid, stream, g, cam, vol, ray, table);
  }
  SFGS_POST_LAUNCH("tsdf_raycast", stream, 0);
  return SFGS_OK;
}
