// pointcloud.hip -- depth maps -> ONE merged point cloud on the device: the reference's depth_to_point_cloud per view
// (evaluate_gs_geometry.py:132-215) and its np.vstack over the views (:776), without a host read per view.
//   append, three launches per view (no kernel waits for another workgroup: a launch is cheaper than a hang):
//     1. pc_count_kernel    a workgroup owns PC_THREADS consecutive pixels and writes how many of them are used;
//     2. scan_sums_kernel   (scan.h) ONE workgroup scans the counts exclusively, PC_SCAN_THREADS at a time with a carry that starts
//                           at the cloud's running total (the state word), leaves every workgroup's first ROW and advances the total;
//     3. pc_scatter_kernel  recomputes validity, ranks the used pixels inside the workgroup (ballot + one LDS word per wave),
//                           unprojects them (geo_unproject.h: geometry.hip's float64 sequence) into LDS and copies the
//                           workgroup's run of rows out with consecutive lanes on consecutive words. Colours alike.
//     Rows keep the view's row-major pixel order, a view's rows follow the previous view's: the buffer is the vstack.
//     A row at or beyond `capacity` is not written; the state counts it all the same.
//   bounds, two launches: per-workgroup minima / maxima of the stored rows, then one workgroup folds them, a wave per output.
//     No float atomics. NaN propagates as in numpy's min / max.
// Every index is range-checked before it is used: a pixel against H * W before its load, a row against capacity before its store.
// The kernels have no profiler ids (the id list of sfgs_profile_kernel_name is closed by the loss kernels).
#include "sfgs_internal.h"
#include "geo_unproject.h"
#include "scan.h"

#include <math.h>

namespace sfgs {

constexpr int PC_THREADS = 256;            // pixels per workgroup of the count and scatter kernels
constexpr int PC_WAVES = PC_THREADS / 64;
constexpr int PC_SCAN_THREADS = 1024;      // counts the scan kernel takes per round of its loop (tests size a view by it)
static_assert(PC_SCAN_THREADS == SCAN_TOP_THREADS, "the scan's round is scan.h's");
constexpr int PC_BOUNDS_MAX_BLOCKS = 1024;

struct PcView {
  GeoCamera cam;
  int H, W;
};

__global__ void __launch_bounds__(PC_THREADS)
pc_count_kernel(const float* __restrict__ depth, const unsigned char* __restrict__ mask, long long P,
                unsigned long long* __restrict__ blk) {
  __shared__ unsigned wave_n[PC_WAVES];
  const long long p = (long long)blockIdx.x * PC_THREADS + threadIdx.x;
  float d = 0.f;
  const bool used = p < P && geo_pixel_used(depth, mask, p, &d);
  const unsigned long long b = __ballot(used);
  if (lane_id() == 0) wave_n[threadIdx.x >> 6] = (unsigned)__popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned n = 0;
#pragma unroll
    for (int w = 0; w < PC_WAVES; ++w) n += wave_n[w];
    blk[blockIdx.x] = n;
  }
}

template <bool COLORS>
__global__ void __launch_bounds__(PC_THREADS)
pc_scatter_kernel(const float* __restrict__ depth, const unsigned char* __restrict__ mask, const float* __restrict__ image,
                  PcView v, const unsigned long long* __restrict__ blk, double* __restrict__ points,
                  unsigned char* __restrict__ colors, long long capacity) {
  __shared__ unsigned wave_n[PC_WAVES];
  __shared__ double srow[PC_THREADS * 3];
  __shared__ unsigned char scol[COLORS ? PC_THREADS * 3 : 1];
  const long long P = (long long)v.H * v.W;
  const long long p = (long long)blockIdx.x * PC_THREADS + threadIdx.x;
  float d = 0.f;
  const bool used = p < P && geo_pixel_used(depth, mask, p, &d);
  const unsigned long long b = __ballot(used);
  const unsigned lane = lane_id(), wave = threadIdx.x >> 6;
  if (lane == 0) wave_n[wave] = (unsigned)__popcll(b);
  __syncthreads();
  unsigned rank = (unsigned)__popcll(b & ((1ull << lane) - 1ull)), n = 0;
#pragma unroll
  for (int w = 0; w < PC_WAVES; ++w) {
    if (w < (int)wave) rank += wave_n[w];
    n += wave_n[w];
  }
  if (used) {                              // rank < n <= PC_THREADS
    const int row = (int)(p / v.W), col = (int)(p - (long long)row * v.W);
    double w[3];
    geo_unproject(v.cam, row, col, d, w);
    srow[3 * rank] = w[0]; srow[3 * rank + 1] = w[1]; srow[3 * rank + 2] = w[2];
    if (COLORS) {
#pragma unroll
      for (int c = 0; c < 3; ++c) scol[3 * rank + c] = fq_byte(image[(long long)c * P + p]);
    }
  }
  __syncthreads();
  const unsigned long long first = blk[blockIdx.x];
  if (first >= (unsigned long long)capacity) return;
  const unsigned long long room = (unsigned long long)capacity - first;
  const unsigned words = 3u * (room < n ? (unsigned)room : n);   // the rows of this workgroup that fit, as words
  for (unsigned k = threadIdx.x; k < words; k += PC_THREADS) points[first * 3ull + k] = srow[k];
  if (COLORS)
    for (unsigned k = threadIdx.x; k < words; k += PC_THREADS) colors[first * 3ull + k] = scol[k];
}

// numpy's min / max: a NaN on either side gives NaN
__device__ __forceinline__ double pc_min(double m, double x) { return (x < m || x != x) ? x : m; }
__device__ __forceinline__ double pc_max(double m, double x) { return (x > m || x != x) ? x : m; }

// part: [6][gridDim.x] = min x, y, z, max x, y, z over the rows this workgroup strides over
__global__ void __launch_bounds__(PC_THREADS)
pc_bounds_kernel(const double* __restrict__ points, const unsigned long long* __restrict__ state, long long capacity,
                 double* __restrict__ part) {
  __shared__ double red[6][PC_THREADS];
  const unsigned long long seen = *state;
  const long long n = seen < (unsigned long long)capacity ? (long long)seen : capacity;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (long long r = (long long)blockIdx.x * PC_THREADS + threadIdx.x; r < n; r += (long long)gridDim.x * PC_THREADS) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double x = points[r * 3 + j];
      lo[j] = pc_min(lo[j], x); hi[j] = pc_max(hi[j], x);
    }
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) { red[j][threadIdx.x] = lo[j]; red[3 + j][threadIdx.x] = hi[j]; }
  __syncthreads();
  for (int w = PC_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        red[j][threadIdx.x] = pc_min(red[j][threadIdx.x], red[j][threadIdx.x + w]);
        red[3 + j][threadIdx.x] = pc_max(red[3 + j][threadIdx.x], red[3 + j][threadIdx.x + w]);
      }
    }
    __syncthreads();
  }
  if (threadIdx.x < 6) part[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = red[threadIdx.x][0];
}

// one wave per output: lane l folds partials l, l + 64, ..., the wave folds its lanes (a minimum does not depend on the order)
__global__ void __launch_bounds__(6 * 64)
pc_bounds_final_kernel(const double* __restrict__ part, int blocks, double* __restrict__ out6) {
  const int q = threadIdx.x >> 6;
  const bool is_min = q < 3;
  double m = is_min ? INFINITY : -INFINITY;
  for (int b = (int)lane_id(); b < blocks; b += 64) {
    const double x = part[(size_t)q * blocks + b];
    m = is_min ? pc_min(m, x) : pc_max(m, x);
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const double x = __shfl_down(m, d);
    m = is_min ? pc_min(m, x) : pc_max(m, x);
  }
  if (lane_id() == 0) out6[q] = m;
}

}  // namespace sfgs

using namespace sfgs;

namespace {

inline long long pc_blocks(long long P) { return (P + PC_THREADS - 1) / PC_THREADS; }
constexpr size_t PC_BOUNDS_BYTES = (size_t)6 * PC_BOUNDS_MAX_BLOCKS * 8;

// Every refusal of this file is SFGS_E_ARG: the caller made the call wrong, nothing was launched.
int pc_check_raster(const char* what, int32_t H, int32_t W) {
  SFGS_REQUIRE(H > 0 && W > 0, SFGS_E_ARG, "%s: H %d, W %d", what, H, W);
  SFGS_REQUIRE((long long)H * W <= (1ll << 30), SFGS_E_ARG, "%s: H * W must not exceed 2^30, got %d x %d", what, H, W);
  return SFGS_OK;
}

size_t pc_scratch_bytes(int32_t H, int32_t W) {
  const size_t counts = align_up((size_t)pc_blocks((long long)H * W) * 8, 256);
  return counts > PC_BOUNDS_BYTES ? counts : PC_BOUNDS_BYTES;
}

}  // namespace

extern "C" size_t sfgs_pointcloud_scratch_bytes(int32_t H, int32_t W) {
  if (pc_check_raster("sfgs_pointcloud_scratch_bytes", H, W)) return 0;
  return pc_scratch_bytes(H, W);
}

extern "C" int sfgs_pointcloud_append(const SfgsPointCloudViewArgs* a, double* points, unsigned char* colors, int64_t capacity,
                                      unsigned long long* state, void* scratch, size_t scratch_bytes, void* stream_) {
  SFGS_REQUIRE(a, SFGS_E_ARG, "NULL SfgsPointCloudViewArgs");
  SFGS_REQUIRE(a->struct_size == sizeof(SfgsPointCloudViewArgs), SFGS_E_ARG, "SfgsPointCloudViewArgs.struct_size %u, expected %zu",
               a->struct_size, sizeof(SfgsPointCloudViewArgs));
  if (const int rc = pc_check_raster("SfgsPointCloudViewArgs", a->H, a->W)) return rc;
  SFGS_REQUIRE(a->focal_x != 0.0 && a->focal_y != 0.0, SFGS_E_ARG, "SfgsPointCloudViewArgs: focal %g, %g", a->focal_x, a->focal_y);
  SFGS_REQUIRE(capacity >= 0, SFGS_E_ARG, "sfgs_pointcloud_append: capacity %lld", (long long)capacity);
  SFGS_REQUIRE(a->depth && points && state && scratch, SFGS_E_ARG, "NULL argument");
  SFGS_REQUIRE((a->image == nullptr) == (colors == nullptr), SFGS_E_ARG,
               "sfgs_pointcloud_append: SfgsPointCloudViewArgs.image and colors come together");
  const size_t need = pc_scratch_bytes(a->H, a->W);
  SFGS_REQUIRE(scratch_bytes >= need, SFGS_E_ARG, "pointcloud scratch too small: %zu < %zu", scratch_bytes, need);
  PcView v;
  for (int i = 0; i < 9; ++i) v.cam.M[i] = a->M[i];
  for (int i = 0; i < 3; ++i) { v.cam.c[i] = a->c[i]; v.cam.origin[i] = a->origin[i]; }
  v.cam.cx_pix = a->cx_pix; v.cam.cy_pix = a->cy_pix; v.cam.focal_x = a->focal_x; v.cam.focal_y = a->focal_y;
  v.H = a->H; v.W = a->W;
  hipStream_t stream = (hipStream_t)stream_;
  const long long P = (long long)a->H * a->W, nblk = pc_blocks(P);
  unsigned long long* blk = (unsigned long long*)scratch;
  const dim3 grid((unsigned)nblk), block(PC_THREADS);
  hipLaunchKernelGGL(pc_count_kernel, grid, block, 0, stream, a->depth, a->mask, P, blk);
  SFGS_POST_LAUNCH("pc_count", stream, 0);
  // blk[b]: count -> first row of workgroup b; *state: rows seen before this view -> after it (carry in and total out: one word)
  hipLaunchKernelGGL(scan_sums_kernel<unsigned long long>, dim3(1), dim3(PC_SCAN_THREADS), 0, stream, blk, nblk, 1,
                     (const unsigned long long*)state, state);
  SFGS_POST_LAUNCH("pc_scan", stream, 0);
  if (colors)
    hipLaunchKernelGGL(pc_scatter_kernel<true>, grid, block, 0, stream, a->depth, a->mask, a->image, v,
                       (const unsigned long long*)blk, points, colors, (long long)capacity);
  else
    hipLaunchKernelGGL(pc_scatter_kernel<false>, grid, block, 0, stream, a->depth, a->mask, a->image, v,
                       (const unsigned long long*)blk, points, colors, (long long)capacity);
  SFGS_POST_LAUNCH("pc_scatter", stream, 0);
  return SFGS_OK;
}

extern "C" int sfgs_pointcloud_bounds(const double* points, const unsigned long long* state, int64_t capacity, double* out6,
                                      void* scratch, size_t scratch_bytes, void* stream_) {
  SFGS_REQUIRE(capacity >= 0, SFGS_E_ARG, "sfgs_pointcloud_bounds: capacity %lld", (long long)capacity);
  SFGS_REQUIRE(points && state && out6 && scratch, SFGS_E_ARG, "NULL argument");
  SFGS_REQUIRE(scratch_bytes >= PC_BOUNDS_BYTES, SFGS_E_ARG, "pointcloud scratch too small: %zu < %zu", scratch_bytes,
               PC_BOUNDS_BYTES);
  hipStream_t stream = (hipStream_t)stream_;
  const long long want = pc_blocks(capacity);
  const int blocks = (int)(want < 1 ? 1 : want < PC_BOUNDS_MAX_BLOCKS ? want : PC_BOUNDS_MAX_BLOCKS);
  hipLaunchKernelGGL(pc_bounds_kernel, dim3((unsigned)blocks), dim3(PC_THREADS), 0, stream, points, state, (long long)capacity,
                     (double*)scratch);
  SFGS_POST_LAUNCH("pc_bounds", stream, 0);
  hipLaunchKernelGGL(pc_bounds_final_kernel, dim3(1), dim3(6 * 64), 0, stream, (const double*)scratch, blocks, out6);
  SFGS_POST_LAUNCH("pc_bounds_final", stream, 0);
  return SFGS_OK;
}
