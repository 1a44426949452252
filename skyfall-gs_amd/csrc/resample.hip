// resample.hip -- create_offset_gt (reference train.py:64-77) applied to mask * original_image (train.py:207, 214-215; :770-771 in
// the IDU episode): the ground truth sampled where the jittered rays of SfgsFrame.subpixel_offset went. The reference builds a
// pixel grid on the host every iteration (np.meshgrid of Python ranges, stack, cast, upload), normalises it, and hands it to
// grid_sample(bilinear, padding_mode="border", align_corners=True). Here: ONE launch, one thread per output pixel (x fastest),
// the pixel's coordinate from its index, include/sfgs.h spells the float32 sequence.
//   offsets: one 8-byte load per lane, consecutive lanes consecutive addresses; stores: one dword per lane and channel, coalesced;
//   taps: |offset| <= 0.5 in training, so a wave's four tap rows are the 64 (+1) floats under it and the row below -- neighbouring
//   lanes read neighbouring addresses, served by L1 / L2. The mask's four taps are loaded once and shared by the channels.
// Bytes the algorithm needs: (2 + C + C + [1]) * 4 * H * W. No LDS, no atomics: deterministic by construction.
// The kernel has no profiler id (the id list of sfgs_profile_kernel_name is closed by the loss kernels and its length is pinned);
// tools/bench_resample.py takes its time from an event pair, the tests count its launches with torch.profiler.
#include "sfgs_internal.h"

namespace sfgs {

constexpr int RS_THREADS = 256;
enum { RS_MASK_NONE = 0, RS_MASK_SCALAR = 1, RS_MASK_PLANE = 2 };
// the (ox, oy) pair of a pixel: 8 bytes, aligned like the floats it is made of (a view may start at an odd float)
typedef float rs_v2f __attribute__((ext_vector_type(2), aligned(4)));

// clamp(t, 0, hi) as torch's device clip_coordinates orders it -- min(hi, max(t, 0)) with max / min that drop a NaN:
// NaN and -inf -> 0, +inf -> hi
__device__ __forceinline__ float rs_clip(float t, float hi) {
  t = t > 0.f ? t : 0.f;
  return t < hi ? t : hi;
}

template <int C, int MASK>
__global__ void __launch_bounds__(RS_THREADS)
resample_gt_kernel(const float* __restrict__ src, const float* __restrict__ mask, const float* __restrict__ offset, int H, int W,
                   float* __restrict__ out) {
  const unsigned P = (unsigned)H * (unsigned)W;                       // C * H * W < 2^31 (checked by the host)
  const unsigned p = blockIdx.x * (unsigned)RS_THREADS + threadIdx.x;
  if (p >= P) return;
  const unsigned y = p / (unsigned)W, x = p - y * (unsigned)W;
  const rs_v2f o = reinterpret_cast<const rs_v2f*>(offset)[p];
  const float u = rs_clip((float)x + o.x, (float)(W - 1)), v = rs_clip((float)y + o.y, (float)(H - 1));
  int x0 = (int)u, y0 = (int)v;                                       // u, v >= 0: truncation is floor
  x0 = x0 < W - 1 ? x0 : W - 1;                                       // (float)(W - 1) rounds up for some W > 2^24: the index
  y0 = y0 < H - 1 ? y0 : H - 1;                                       // stays inside the plane whatever the float says
  const float fx = u - (float)x0, fy = v - (float)y0;                 // exact
  const int x1 = x0 + 1 < W ? x0 + 1 : W - 1, y1 = y0 + 1 < H ? y0 + 1 : H - 1;   // at u = W - 1 the neighbour's weight is 0
  const float gx = 1.0f - fx, gy = 1.0f - fy;
  const float w00 = gx * gy, w01 = fx * gy, w10 = gx * fy, w11 = fx * fy;
  const unsigned i00 = (unsigned)y0 * W + x0, i01 = (unsigned)y0 * W + x1, i10 = (unsigned)y1 * W + x0, i11 = (unsigned)y1 * W + x1;
  float m00 = 1.0f, m01 = 1.0f, m10 = 1.0f, m11 = 1.0f;
  if (MASK == RS_MASK_SCALAR) m00 = m01 = m10 = m11 = mask[0];
  if (MASK == RS_MASK_PLANE) { m00 = mask[i00]; m01 = mask[i01]; m10 = mask[i10]; m11 = mask[i11]; }
  float t[C][4];
#pragma unroll
  for (int c = 0; c < C; ++c) {                                       // every tap in flight before the first use
    const float* __restrict__ s = src + (size_t)c * P;
    t[c][0] = s[i00]; t[c][1] = s[i01]; t[c][2] = s[i10]; t[c][3] = s[i11];
  }
#pragma unroll
  for (int c = 0; c < C; ++c) {
    float a = t[c][0], b = t[c][1], d = t[c][2], e = t[c][3];
    if (MASK != RS_MASK_NONE) { a = m00 * a; b = m01 * b; d = m10 * d; e = m11 * e; }   // the reference's mask * image, per tap
    out[(size_t)c * P + p] = ((a * w00 + b * w01) + d * w10) + e * w11;
  }
}

}  // namespace sfgs

using namespace sfgs;

namespace {

template <int C>
void rs_launch(int mask_mode, unsigned blocks, hipStream_t stream, const SfgsResampleArgs* a, float* out) {
  const dim3 grid(blocks), block(RS_THREADS);
  if (mask_mode == RS_MASK_PLANE)
    hipLaunchKernelGGL((resample_gt_kernel<C, RS_MASK_PLANE>), grid, block, 0, stream, a->src, a->mask, a->offset, a->H, a->W, out);
  else if (mask_mode == RS_MASK_SCALAR)
    hipLaunchKernelGGL((resample_gt_kernel<C, RS_MASK_SCALAR>), grid, block, 0, stream, a->src, a->mask, a->offset, a->H, a->W, out);
  else
    hipLaunchKernelGGL((resample_gt_kernel<C, RS_MASK_NONE>), grid, block, 0, stream, a->src, a->mask, a->offset, a->H, a->W, out);
}

}  // namespace

extern "C" int sfgs_resample_gt(const SfgsResampleArgs* a, float* out, void* stream_) {
  SFGS_REQUIRE(a, SFGS_E_ARG, "NULL SfgsResampleArgs");
  SFGS_REQUIRE(a->struct_size == sizeof(SfgsResampleArgs), SFGS_E_ARG, "SfgsResampleArgs.struct_size %u, expected %zu",
               a->struct_size, sizeof(SfgsResampleArgs));
  SFGS_REQUIRE(a->C >= 1 && a->C <= 4, SFGS_E_ARG, "SfgsResampleArgs.C %d is not 1 ... 4", a->C);
  SFGS_REQUIRE(a->H >= 2 && a->W >= 2, SFGS_E_ARG, "SfgsResampleArgs: H %d, W %d; both must be at least 2", a->H, a->W);
  const long long P = (long long)a->H * a->W;
  SFGS_REQUIRE(a->C * P < (1ll << 31), SFGS_E_UNSUPPORTED, "SfgsResampleArgs: C * H * W must stay below 2^31, got %d x %d x %d",
               a->C, a->H, a->W);
  SFGS_REQUIRE(a->mask_elems == 0 || a->mask_elems == 1 || a->mask_elems == P, SFGS_E_ARG,
               "SfgsResampleArgs.mask_elems %lld is neither 0, 1 nor H * W", (long long)a->mask_elems);
  SFGS_REQUIRE((a->mask_elems == 0) == (a->mask == nullptr), SFGS_E_ARG, "SfgsResampleArgs.mask and mask_elems disagree");
  SFGS_REQUIRE(a->src && a->offset && out, SFGS_E_ARG, "NULL argument");
  const uintptr_t s0 = (uintptr_t)a->src, o0 = (uintptr_t)out, nbytes = (uintptr_t)(a->C * P) * 4u;
  SFGS_REQUIRE(o0 + nbytes <= s0 || s0 + nbytes <= o0, SFGS_E_ARG, "SfgsResampleArgs: out overlaps src");
  hipStream_t stream = (hipStream_t)stream_;
  const int mask_mode = a->mask_elems == 0 ? RS_MASK_NONE : (a->mask_elems == 1 ? RS_MASK_SCALAR : RS_MASK_PLANE);
  const unsigned blocks = (unsigned)((P + RS_THREADS - 1) / RS_THREADS);
  switch (a->C) {
    case 1: rs_launch<1>(mask_mode, blocks, stream, a, out); break;
    case 2: rs_launch<2>(mask_mode, blocks, stream, a, out); break;
    case 3: rs_launch<3>(mask_mode, blocks, stream, a, out); break;
    default: rs_launch<4>(mask_mode, blocks, stream, a, out); break;
  }
  SFGS_POST_LAUNCH("resample_gt", stream, 0);
  return SFGS_OK;
}
