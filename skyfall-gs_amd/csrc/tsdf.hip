// tsdf.hip -- depth views -> a truncated signed distance volume -> a triangle soup: the surface the other geometry products
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
//     2. tsdf_scan_kernel   ONE workgroup scans the counts exclusively, 1024 at a time with a carry, and leaves the total in *state;
//     3. tsdf_emit_kernel   recomputes the cells, ranks their triangles inside the workgroup and writes the workgroup's run.
//     The soup is ordered by cell, tetrahedron, triangle. A row at or beyond `capacity` is not written; the state counts it.
// Every index is range-checked before it is used: a voxel against the volume before its load and store, a pixel against its view's
// H x W (on the doubles) before its load, a cell against the cell grid before its eight corners, a row against capacity.
// No profiler ids.
#include "sfgs_internal.h"
#include "tsdf_math.h"

#include <math.h>

namespace sfgs {

constexpr int TSDF_THREADS = 256;
constexpr int TSDF_WAVES = TSDF_THREADS / 64;
constexpr int TSDF_BRICK_X = 8, TSDF_BRICK_Y = 8, TSDF_BRICK_Z = 4;     // TSDF_THREADS voxels; a wave is one z-slab of it
constexpr int TSDF_SCAN_THREADS = 1024;
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

// blk[b]: count -> first row of workgroup b; *state = the total (what was there before is not read)
__global__ void __launch_bounds__(TSDF_SCAN_THREADS)
tsdf_scan_kernel(unsigned long long* __restrict__ blk, long long nblk, unsigned long long* __restrict__ state) {
  __shared__ unsigned smem[TSDF_SCAN_THREADS / 64 + 1];
  unsigned long long carry = 0;
  for (long long base = 0; base < nblk; base += TSDF_SCAN_THREADS) {
    const long long i = base + threadIdx.x;
    const unsigned c = i < nblk ? (unsigned)blk[i] : 0u;
    unsigned total;                        // <= TSDF_SCAN_THREADS * TSDF_THREADS * 12 < 2^22
    const unsigned before = block_excl_scan_u32<TSDF_SCAN_THREADS>(c, &total, smem);
    if (i < nblk) blk[i] = carry + before;
    carry += total;
  }
  if (threadIdx.x == 0) *state = carry;
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
  hipLaunchKernelGGL(tsdf_scan_kernel, dim3(1), dim3(TSDF_SCAN_THREADS), 0, stream, blk, nblk, state);
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
