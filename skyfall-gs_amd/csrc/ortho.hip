// ortho.hip -- the true orthophoto on the DSM's grid from the rendered views (evaluate_gs_geometry.py:736-765 renders depth AND
// colour per camera; geometry.hip keeps the depth): per cell the colour of the HIGHEST point that fell into it, two kernels.
//   1. ortho_accumulate_kernel, once per view: a thread per pixel (striding when the view has more than 2^18); the pixel rule,
//      the float64 unprojection and the cell rule are geometry.hip's (geo_unproject.h, one device function each, the
//      expressions moved verbatim). Height first, colour second, the view's tag last are
//      packed into ONE 64-bit key and the cell takes its maximum with an integer atomic: the winner of a cell is the maximum
//      over (float32 height, r, g, b, tag), lexicographically. No float atomics, no second pass, no retained images: any view
//      order gives the same bits.
//        bits 63-32  ortho_key32(float32(up)): order preserving, no number maps to 0 (0 = an empty cell)
//        bits 31-8   r, g, b by sfgs_frame_quantize's rule (fq_byte)
//        bits 7-0    the view's tag, 1 ... 255
//      The cell is read with a plain load first and the atomic is skipped when the point cannot win. A cell only ever grows
//      and a stale value (L1, another XCD's L2) can only be LOWER than the true one, so a skipped point could never have won.
//   2. ortho_resolve_kernel, one launch: a thread per cell (striding beyond 2^17 cells) unpacks the key; an EMPTY cell may take
//      the maximum key among the non-empty cells of its (2 fill + 1)^2 window (clipped to the grid; one pass: donated values
//      do not propagate). The histogram of winning tags goes through 256 LDS counters per workgroup, non-zero bins then to
//      `coverage`.
// Every index is range-checked before it is used: a pixel against H * W before its loads, a cell before its atomic (geo_cell),
// a window cell against the grid before its load. The kernels have no profiler ids.
#include "sfgs_internal.h"
#include "geo_unproject.h"

#include <math.h>

namespace sfgs {

constexpr int ORTHO_THREADS = 256;       // = the bins of the tag histogram: one LDS counter per thread
constexpr int ORTHO_MAX_FILL = 3;
// Both kernels stride over their pixels / cells with a capped grid, so that the atomics on the FEW shared words -- the point
// counter, the 256 coverage bins -- are one per workgroup (and bin), not one per wave: at most this many per launch.
constexpr int ORTHO_ACC_MAX_BLOCKS = 1024;
constexpr int ORTHO_RESOLVE_MAX_BLOCKS = 512;

struct OrthoView {
  GeoCamera cam;
  double xoff, yoff_top, res;
  int H, W, xsize, ysize;
  unsigned tag;
};

// order-preserving key of a float32's bits: a < b <=> key(a) < key(b); no number has key 0. The 32-bit analogue of dsm_key.
__device__ __forceinline__ unsigned ortho_key32(unsigned b) { return (b >> 31) ? ~b : (b | 0x80000000u); }
__device__ __forceinline__ unsigned ortho_unkey32(unsigned k) { return (k >> 31) ? (k & 0x7fffffffu) : ~k; }

__global__ void __launch_bounds__(ORTHO_THREADS)
ortho_accumulate_kernel(const float* __restrict__ depth, const unsigned char* __restrict__ mask, const float* __restrict__ image,
                        OrthoView v, unsigned long long* acc, unsigned long long* __restrict__ num_points) {
  __shared__ unsigned block_n;
  if (threadIdx.x == 0) block_n = 0u;
  __syncthreads();
  const long long P = (long long)v.H * v.W, stride = (long long)gridDim.x * ORTHO_THREADS;
  unsigned n = 0;                          // the wave's landed points (the same in every lane)
  for (long long base = (long long)blockIdx.x * ORTHO_THREADS; base < P; base += stride) {   // workgroup-uniform trip count
    const long long p = base + threadIdx.x;
    bool landed = false;
    if (p < P) {
      float d;
      if (geo_pixel_used(depth, mask, p, &d)) {
        const int row = (int)(p / v.W), col = (int)(p - (long long)row * v.W);
        double w[3];
        geo_unproject(v.cam, row, col, d, w);
        int gx, gy;
        // a height that is not finite cannot arise from checked inputs; it is dropped, not keyed
        if (fabs(w[2]) < INFINITY && geo_cell(w[0], w[1], v.xoff, v.yoff_top, v.res, v.xsize, v.ysize, &gx, &gy)) {
          landed = true;
          const unsigned hi = ortho_key32(__float_as_uint((float)w[2]));   // (float): round to nearest even
          const unsigned lo = ((unsigned)fq_byte(image[p]) << 24) | ((unsigned)fq_byte(image[P + p]) << 16) |
                              ((unsigned)fq_byte(image[2 * P + p]) << 8) | v.tag;
          const unsigned long long key = ((unsigned long long)hi << 32) | lo;
          unsigned long long* cell = &acc[(size_t)gy * v.xsize + gx];
          if (*cell < key) atomicMax(cell, key);
        }
      }
    }
    n += (unsigned)__popcll(__ballot(landed));
  }
  // ONE atomic on the counter per workgroup: a single word takes about a hundred atomics per microsecond on this chip, and one
  // per wave (dsm_accumulate_kernel's count) is 16384 of them for a 1024 x 1024 view (profiles/r19_ortho_ab.txt)
  if (lane_id() == 0 && n) atomicAdd(&block_n, n);
  __syncthreads();
  if (threadIdx.x == 0 && block_n) atomicAdd(num_points, (unsigned long long)block_n);
}

__global__ void __launch_bounds__(ORTHO_THREADS)
ortho_resolve_kernel(const unsigned long long* __restrict__ acc, int xsize, int ysize, int fill, unsigned char* __restrict__ rgb,
                     float* __restrict__ height, unsigned char* __restrict__ source, unsigned char* __restrict__ state,
                     unsigned long long* __restrict__ coverage) {
  __shared__ unsigned hist[ORTHO_THREADS];
  hist[threadIdx.x] = 0u;
  __syncthreads();
  const long long cells = (long long)xsize * ysize, stride = (long long)gridDim.x * ORTHO_THREADS;
  for (long long i = (long long)blockIdx.x * ORTHO_THREADS + threadIdx.x; i < cells; i += stride) {
    unsigned long long k = acc[i];
    unsigned st = k ? 1u : 0u;
    if (!k && fill > 0) {
      const int gy = (int)(i / xsize), gx = (int)(i - (long long)gy * xsize);
      const int y0 = gy - fill < 0 ? 0 : gy - fill, y1 = gy + fill >= ysize ? ysize - 1 : gy + fill;
      const int x0 = gx - fill < 0 ? 0 : gx - fill, x1 = gx + fill >= xsize ? xsize - 1 : gx + fill;
      for (int y = y0; y <= y1; ++y)
        for (int x = x0; x <= x1; ++x) {
          const unsigned long long t = acc[(size_t)y * xsize + x];
          k = t > k ? t : k;
        }
      if (k) st = 2u;
    }
    const unsigned lo = (unsigned)k;
    rgb[3 * i] = (unsigned char)(lo >> 24);
    rgb[3 * i + 1] = (unsigned char)(lo >> 16);
    rgb[3 * i + 2] = (unsigned char)(lo >> 8);
    height[i] = k ? __uint_as_float(ortho_unkey32((unsigned)(k >> 32))) : __uint_as_float(0x7fc00000u);
    source[i] = (unsigned char)lo;       // a key's tag is 1 ... 255, an empty cell's 0
    state[i] = (unsigned char)st;
    atomicAdd(&hist[lo & 0xffu], 1u);
  }
  __syncthreads();
  const unsigned n = hist[threadIdx.x];
  if (n) atomicAdd(&coverage[threadIdx.x], (unsigned long long)n);
}

}  // namespace sfgs

using namespace sfgs;

namespace {

inline unsigned ortho_blocks(long long n, int cap) {
  const long long want = (n + ORTHO_THREADS - 1) / ORTHO_THREADS;
  return (unsigned)(want < cap ? want : cap);
}

// sfgs_dsm_accumulate's limits and status codes
int ortho_check_grid(int32_t xsize, int32_t ysize) {
  SFGS_REQUIRE(xsize > 0 && ysize > 0, SFGS_E_ARG, "ortho grid: xsize %d, ysize %d", xsize, ysize);
  SFGS_REQUIRE((long long)xsize * ysize <= (1ll << 28), SFGS_E_UNSUPPORTED, "ortho grid: xsize * ysize must not exceed 2^28, got %d x %d",
               xsize, ysize);
  return SFGS_OK;
}

}  // namespace

extern "C" int sfgs_ortho_accumulate(const SfgsOrthoViewArgs* a, void* acc, unsigned long long* num_points, void* stream_) {
  SFGS_REQUIRE(a, SFGS_E_ARG, "NULL SfgsOrthoViewArgs");
  SFGS_REQUIRE(a->struct_size == sizeof(SfgsOrthoViewArgs), SFGS_E_ARG, "SfgsOrthoViewArgs.struct_size %u, expected %zu",
               a->struct_size, sizeof(SfgsOrthoViewArgs));
  SFGS_REQUIRE(a->H > 0 && a->W > 0, SFGS_E_ARG, "SfgsOrthoViewArgs: H %d, W %d", a->H, a->W);
  SFGS_REQUIRE((long long)a->H * a->W <= (1ll << 30), SFGS_E_UNSUPPORTED, "SfgsOrthoViewArgs: H * W must not exceed 2^30, got %d x %d",
               a->H, a->W);
  if (const int rc = ortho_check_grid(a->xsize, a->ysize)) return rc;
  SFGS_REQUIRE(a->tag >= 1 && a->tag <= 255, SFGS_E_ARG, "SfgsOrthoViewArgs.tag %d: 1 ... 255", a->tag);
  SFGS_REQUIRE(a->resolution > 0.0 && a->focal_x != 0.0 && a->focal_y != 0.0, SFGS_E_ARG,
               "SfgsOrthoViewArgs: resolution %g, focal %g, %g", a->resolution, a->focal_x, a->focal_y);
  SFGS_REQUIRE(a->depth && a->image && acc && num_points, SFGS_E_ARG, "NULL argument");
  OrthoView v;
  for (int i = 0; i < 9; ++i) v.cam.M[i] = a->M[i];
  for (int i = 0; i < 3; ++i) { v.cam.c[i] = a->c[i]; v.cam.origin[i] = a->origin[i]; }
  v.cam.cx_pix = a->cx_pix; v.cam.cy_pix = a->cy_pix; v.cam.focal_x = a->focal_x; v.cam.focal_y = a->focal_y;
  v.xoff = a->xoff; v.yoff_top = a->yoff_top; v.res = a->resolution;
  v.H = a->H; v.W = a->W; v.xsize = a->xsize; v.ysize = a->ysize; v.tag = (unsigned)a->tag;
  hipStream_t stream = (hipStream_t)stream_;
  hipLaunchKernelGGL(ortho_accumulate_kernel, dim3(ortho_blocks((long long)a->H * a->W, ORTHO_ACC_MAX_BLOCKS)),
                     dim3(ORTHO_THREADS), 0, stream, a->depth, a->mask, a->image, v, (unsigned long long*)acc, num_points);
  SFGS_POST_LAUNCH("ortho_accumulate", stream, 0);
  return SFGS_OK;
}

extern "C" int sfgs_ortho_resolve(int32_t xsize, int32_t ysize, int32_t fill, const void* acc, unsigned char* rgb, float* height,
                                  unsigned char* source, unsigned char* state, unsigned long long* coverage, void* stream_) {
  if (const int rc = ortho_check_grid(xsize, ysize)) return rc;
  SFGS_REQUIRE(fill >= 0 && fill <= ORTHO_MAX_FILL, SFGS_E_ARG, "sfgs_ortho_resolve: fill %d: 0 ... %d", fill, ORTHO_MAX_FILL);
  SFGS_REQUIRE(acc && rgb && height && source && state && coverage, SFGS_E_ARG, "NULL argument");
  hipStream_t stream = (hipStream_t)stream_;
  hipLaunchKernelGGL(ortho_resolve_kernel, dim3(ortho_blocks((long long)xsize * ysize, ORTHO_RESOLVE_MAX_BLOCKS)),
                     dim3(ORTHO_THREADS), 0, stream, (const unsigned long long*)acc, xsize, ysize, fill, rgb, height, source, state,
                     coverage);
  SFGS_POST_LAUNCH("ortho_resolve", stream, 0);
  return SFGS_OK;
}
