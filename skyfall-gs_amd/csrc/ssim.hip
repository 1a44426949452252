// ssim.hip -- fused SSIM forward/backward for gfx950. Replaces fused_ssim.fused_ssim(img1, img2)
// (reference call sites train.py:222,778; semantics == utils/loss_utils.py:23-63: 11x11 Gaussian window
// sigma 1.5, zero "same" padding, C1 = 0.01^2, C2 = 0.03^2, mean over all elements, gradient w.r.t. img1).
//
// One 32 x 22 output tile per 256-thread workgroup: the 42 x 32 input halos of both images are staged in LDS, the
// separable window runs as a horizontal pass into LDS followed by a vertical pass, both with REGISTER sliding windows
// (a thread produces 4 (3) neighbouring outputs from 14 (13) staged values: 3.5-4.3 LDS reads per output and moment
// instead of 11); 5 moments: mu1, mu2, E[x^2], E[y^2], E[xy]. Every output is the same ascending-k fma chain as a
// direct 11-tap sum. HBM traffic: forward reads 2 planes (the halo re-reads hit L2) and writes 3 partial-derivative
// maps (training) -- backward reads those 3 maps + 2 planes, writes 1. The mean is reduced without float atomics
// (per-block partials + a fixed-order final sum), so the loss is bit-reproducible.
#include "ssim_tile.h"

namespace sfgs {

__constant__ float SSIM_W[11] = SSIM_WINDOW_VALUES;

__global__ void __launch_bounds__(256)
ssim_fwd_kernel(const float* __restrict__ img1, const float* __restrict__ img2, int H, int W, int tiles_x, int tiles_y,
                float* __restrict__ ssim_map, float* __restrict__ block_partials, float* __restrict__ dm_dmu1,
                float* __restrict__ dm_dsig1, float* __restrict__ dm_dsig12) {
  __shared__ float s1[SINY][SPITCH], s2[SINY][SPITCH];   // 11.3 KB of staged inputs
  __shared__ float hz[5][SINY][ST];                       // 20.5 KB of horizontal-pass results
  __shared__ float red[4];
  const SsimTile T = ssim_tile(tiles_x, tiles_y);
  const size_t poff = (size_t)T.plane * H * W;
  const uint32_t pbytes = (uint32_t)H * (uint32_t)W * 4u;
  const int x0 = T.x0, y0 = T.y0;
  const int tid = threadIdx.x;
  const WindowWeights ww = window_weights(SSIM_W);
  // staging: every load is issued before the first LDS write, from an address that is always valid (clamped into the
  // image); the zero padding is applied when the value goes to LDS. (A load behind a per-lane condition compiles to
  // load / s_waitcnt vmcnt(0) / ds_write per element: 14 serialised round trips to HBM per tile, 57 % of the wave
  // time parked in waits -- profiles/r5_ssim_sq_counters_before.txt.)
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const HaloLane hl = halo_lane(lane, x0, W);
  float r1[SROUNDS], r2[SROUNDS];
  bool yin[SROUNDS];
  const rsrc_t b1 = plane_rsrc(img1 + poff, pbytes), b2 = plane_rsrc(img2 + poff, pbytes);
#pragma unroll
  for (int r = 0; r < SROUNDS; ++r) {
    const uint32_t row = halo_row(4 * r + wv, y0, H, W, yin[r]);
    r1[r] = bload(b1, hl.xoff, row);
    r2[r] = bload(b2, hl.xoff, row);
  }
  if (lane < SIN) {
#pragma unroll
    for (int r = 0; r < SROUNDS; ++r) {
      const bool in = hl.xin && yin[r];
      s1[4 * r + wv][lane] = in ? r1[r] : 0.f;
      s2[4 * r + wv][lane] = in ? r2[r] : 0.f;
    }
  }
  __syncthreads();
  {  // horizontal pass: thread = (staged row, group of SQ output columns)
    const int ly = tid / (ST / SQ), hx = (tid - ly * (ST / SQ)) * SQ;
    float a[SQ + 10], b[SQ + 10], t[SQ + 10], o[SQ];
#pragma unroll
    for (int k = 0; k < SQ + 10; ++k) { a[k] = s1[ly][hx + k]; b[k] = s2[ly][hx + k]; }
    window<SQ>(ww, a, o);
#pragma unroll
    for (int q = 0; q < SQ; ++q) hz[0][ly][hx + q] = o[q];
    window<SQ>(ww, b, o);
#pragma unroll
    for (int q = 0; q < SQ; ++q) hz[1][ly][hx + q] = o[q];
#pragma unroll
    for (int k = 0; k < SQ + 10; ++k) t[k] = a[k] * a[k];
    window<SQ>(ww, t, o);
#pragma unroll
    for (int q = 0; q < SQ; ++q) hz[2][ly][hx + q] = o[q];
#pragma unroll
    for (int k = 0; k < SQ + 10; ++k) t[k] = b[k] * b[k];
    window<SQ>(ww, t, o);
#pragma unroll
    for (int q = 0; q < SQ; ++q) hz[3][ly][hx + q] = o[q];
#pragma unroll
    for (int k = 0; k < SQ + 10; ++k) t[k] = a[k] * b[k];
    window<SQ>(ww, t, o);
#pragma unroll
    for (int q = 0; q < SQ; ++q) hz[4][ly][hx + q] = o[q];
  }
  __syncthreads();
  // vertical pass: thread = (column, group of SQV output rows); the last group's rows 22, 23 do not exist: their
  // windows read hz rows that were never staged (clamped below) and nothing is written for them
  const int lx = tid & (ST - 1), ly0 = (tid / ST) * SQV;
  float mo[5][SQV];
#pragma unroll
  for (int m = 0; m < 5; ++m) {
    float v[SQV + 10];
#pragma unroll
    for (int k = 0; k < SQV + 10; ++k) v[k] = hz[m][vrow(ly0, k)][lx];
    window<SQV>(ww, v, mo[m]);
  }
  const int gx = x0 + lx;
  const rsrc_t o0 = plane_rsrc(ssim_map + poff, pbytes), o1 = plane_rsrc(dm_dmu1 + poff, pbytes),
               o2 = plane_rsrc(dm_dsig1 + poff, pbytes), o3 = plane_rsrc(dm_dsig12 + poff, pbytes);
  const uint32_t vout = (uint32_t)(ly0 * W + lx) * 4u;   // the thread's first output, relative to the tile origin
  float vsum = 0.f;
#pragma unroll
  for (int q = 0; q < SQV; ++q) {
    const int gy = y0 + ly0 + q;
    const uint32_t sout = (uint32_t)((y0 + q) * W + x0) * 4u;   // tile origin + q rows: scalar
    if (gx < W && gy < H && ly0 + q < STY) {
      const float mu1 = mo[0][q], mu2 = mo[1][q], e11 = mo[2][q], e22 = mo[3][q], e12 = mo[4][q];
      const float mu1sq = mu1 * mu1, mu2sq = mu2 * mu2, mu12 = mu1 * mu2;
      const float sg1 = e11 - mu1sq, sg2 = e22 - mu2sq, sg12 = e12 - mu12;
      const float A1 = 2.f * mu12 + SSIM_C1, A2 = 2.f * sg12 + SSIM_C2;
      const float B1 = mu1sq + mu2sq + SSIM_C1, B2 = sg1 + sg2 + SSIM_C2;
      const float inv = 1.0f / (B1 * B2);
      const float val = A1 * A2 * inv;
      vsum += val;
      if (ssim_map) bstore(val, o0, vout, sout);
      if (dm_dmu1) {
        // partials w.r.t. the three convolution outputs that depend on img1: mu1, E[x^2], E[xy]
        // one division per pixel: 1 / B1 = B2 * inv and 1 / B2 = B1 * inv (an IEEE division is ten VALU instructions
        // and this kernel is VALU-bound)
        const float d_sig1 = -val * (B1 * inv);    // d/d sigma1_sq = -val / B2
        const float d_sig12 = 2.f * A1 * inv;      // d/d sigma12
        bstore(2.f * mu2 * A2 * inv - 2.f * mu1 * val * (B2 * inv) - 2.f * mu1 * d_sig1 - mu2 * d_sig12, o1, vout, sout);
        bstore(d_sig1, o2, vout, sout);
        bstore(d_sig12, o3, vout, sout);
      }
    }
  }
  const float bs = block_sum_256(vsum, red);
  if (tid == 0) block_partials[T.index] = bs;
}

// fixed-order final reduction: mean = sum(partials) / count
__global__ void __launch_bounds__(1024) ssim_mean_kernel(const float* __restrict__ partials, int n, float inv_count,
                                                         float* __restrict__ out) {
  __shared__ double sm[16];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 1024) acc += (double)partials[i];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < 16; ++w) t += sm[w];
    out[0] = (float)(t * (double)inv_count);
  }
}

__global__ void __launch_bounds__(256)
ssim_bwd_kernel(const float* __restrict__ img1, const float* __restrict__ img2, int H, int W, int tiles_x, int tiles_y,
                const float* __restrict__ dm_dmu1, const float* __restrict__ dm_dsig1,
                const float* __restrict__ dm_dsig12, const float* __restrict__ dL_dmean, float inv_count,
                float* __restrict__ dL_dimg1) {
  __shared__ float s[3][SINY][SPITCH];   // 16.9 KB
  __shared__ float hz[3][SINY][ST];      // 12.3 KB
  const SsimTile T = ssim_tile(tiles_x, tiles_y);
  const size_t poff = (size_t)T.plane * H * W;
  const uint32_t pbytes = (uint32_t)H * (uint32_t)W * 4u;
  const int x0 = T.x0, y0 = T.y0;
  const int tid = threadIdx.x;
  const WindowWeights ww = window_weights(SSIM_W);
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const HaloLane hl = halo_lane(lane, x0, W);
  float r0[SROUNDS], r1[SROUNDS], r2[SROUNDS];   // all 24 loads in flight before the first LDS write (see forward)
  bool yin[SROUNDS];
  const rsrc_t m0 = plane_rsrc(dm_dmu1 + poff, pbytes), m1 = plane_rsrc(dm_dsig1 + poff, pbytes),
               m2 = plane_rsrc(dm_dsig12 + poff, pbytes);
#pragma unroll
  for (int r = 0; r < SROUNDS; ++r) {
    const uint32_t row = halo_row(4 * r + wv, y0, H, W, yin[r]);
    r0[r] = bload(m0, hl.xoff, row);
    r1[r] = bload(m1, hl.xoff, row);
    r2[r] = bload(m2, hl.xoff, row);
  }
  // this thread's own pixels are needed last: their loads go out with the halos'
  const int lx = tid & (ST - 1), ly0 = (tid / ST) * SQV;
  const int gx = x0 + lx;
  // (pixels that do not exist load the plane's first pixel: unused)
  const rsrc_t b1 = plane_rsrc(img1 + poff, pbytes), b2 = plane_rsrc(img2 + poff, pbytes),
               og = plane_rsrc(dL_dimg1 + poff, pbytes);
  const uint32_t vout = (uint32_t)(ly0 * W + lx) * 4u;   // the thread's first pixel, relative to the tile origin
  float p1[SQV], p2[SQV];
#pragma unroll
  for (int q = 0; q < SQV; ++q) {
    const bool ok = gx < W && y0 + ly0 + q < H && ly0 + q < STY;
    const uint32_t sout = (uint32_t)((y0 + q) * W + x0) * 4u;
    p1[q] = bload(b1, ok ? vout : 0u, ok ? sout : 0u);
    p2[q] = bload(b2, ok ? vout : 0u, ok ? sout : 0u);
  }
  if (lane < SIN) {
#pragma unroll
    for (int r = 0; r < SROUNDS; ++r) {
      const bool in = hl.xin && yin[r];
      s[0][4 * r + wv][lane] = in ? r0[r] : 0.f;
      s[1][4 * r + wv][lane] = in ? r1[r] : 0.f;
      s[2][4 * r + wv][lane] = in ? r2[r] : 0.f;
    }
  }
  __syncthreads();
  {
    const int ly = tid / (ST / SQ), hx = (tid - ly * (ST / SQ)) * SQ;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      float v[SQ + 10], o[SQ];
#pragma unroll
      for (int k = 0; k < SQ + 10; ++k) v[k] = s[m][ly][hx + k];
      window<SQ>(ww, v, o);
#pragma unroll
      for (int q = 0; q < SQ; ++q) hz[m][ly][hx + q] = o[q];
    }
  }
  __syncthreads();
  float mo[3][SQV];
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    float v[SQV + 10];
#pragma unroll
    for (int k = 0; k < SQV + 10; ++k) v[k] = hz[m][vrow(ly0, k)][lx];
    window<SQV>(ww, v, mo[m]);
  }
  const float scale = dL_dmean[0] * inv_count;
#pragma unroll
  for (int q = 0; q < SQV; ++q) {
    const int gy = y0 + ly0 + q;
    if (gx < W && gy < H && ly0 + q < STY)
      bstore(scale * (mo[0][q] + 2.f * p1[q] * mo[1][q] + p2[q] * mo[2][q]), og, vout, (uint32_t)((y0 + q) * W + x0) * 4u);
  }
}

}  // namespace sfgs

using namespace sfgs;

static inline size_t ssim_nblocks(int B, int C, int H, int W) {
  return (size_t)B * C * ((H + STY - 1) / STY) * ((W + ST - 1) / ST);
}

extern "C" size_t sfgs_ssim_scratch_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t with_grad) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  size_t b = align_up(ssim_nblocks(B, C, H, W) * 4, 256);
  if (with_grad) b += 3 * align_up((size_t)B * C * H * W * 4, 256);
  return b;
}

extern "C" int sfgs_ssim_forward(const float* img1, const float* img2, int32_t B, int32_t C, int32_t H, int32_t W,
                                 float* ssim_map_or_null, float* ssim_mean, void* scratch, size_t scratch_sz,
                                 int32_t with_grad, void* stream_) {
  SFGS_REQUIRE(img1 && img2 && ssim_mean && scratch, SFGS_E_ARG, "NULL argument");
  SFGS_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, SFGS_E_ARG, "bad image shape [%d,%d,%d,%d]", B, C, H, W);
  SFGS_REQUIRE(ssim_nblocks(B, C, H, W) <= (size_t)INT32_MAX, SFGS_E_UNSUPPORTED, "more than 2^31 - 1 tiles of 32 x 22");
  SFGS_REQUIRE((int64_t)H * W < ((int64_t)1 << 30), SFGS_E_UNSUPPORTED, "an image plane of 2^30 pixels or more");
  SFGS_REQUIRE(scratch_sz >= sfgs_ssim_scratch_bytes(B, C, H, W, with_grad), SFGS_E_CAPACITY, "ssim scratch too small");
  hipStream_t stream = (hipStream_t)stream_;
  const size_t nblk = ssim_nblocks(B, C, H, W), plane = align_up((size_t)B * C * H * W * 4, 256);
  float* partials = (float*)scratch;
  char* maps = (char*)scratch + align_up(nblk * 4, 256);
  float* m0 = with_grad ? (float*)maps : nullptr;
  float* m1 = with_grad ? (float*)(maps + plane) : nullptr;
  float* m2 = with_grad ? (float*)(maps + 2 * plane) : nullptr;
  const int tiles_x = (W + ST - 1) / ST, tiles_y = (H + STY - 1) / STY;
  { ProfScope ps_(KID_SSIM_FWD, stream);
    hipLaunchKernelGGL(ssim_fwd_kernel, dim3((unsigned)nblk), dim3(256), 0, stream, img1, img2, H, W, tiles_x, tiles_y,
                       ssim_map_or_null, partials, m0, m1, m2); }
  SFGS_POST_LAUNCH("ssim_fwd", stream, 0);
  { ProfScope ps_(KID_SSIM_MEAN, stream);
    hipLaunchKernelGGL(ssim_mean_kernel, dim3(1), dim3(1024), 0, stream, partials, (int)nblk,
                       1.0f / (float)((double)B * C * H * W), ssim_mean); }
  SFGS_POST_LAUNCH("ssim_mean", stream, 0);
  return SFGS_OK;
}

extern "C" int sfgs_ssim_backward(const float* img1, const float* img2, int32_t B, int32_t C, int32_t H, int32_t W,
                                  const void* scratch, const float* dL_dmean, float* dL_dimg1, void* stream_) {
  SFGS_REQUIRE(img1 && img2 && scratch && dL_dmean && dL_dimg1, SFGS_E_ARG, "NULL argument");
  SFGS_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, SFGS_E_ARG, "bad image shape");
  SFGS_REQUIRE(ssim_nblocks(B, C, H, W) <= (size_t)INT32_MAX && (int64_t)H * W < ((int64_t)1 << 30),
               SFGS_E_UNSUPPORTED, "image too large");
  hipStream_t stream = (hipStream_t)stream_;
  const size_t nblk = ssim_nblocks(B, C, H, W), plane = align_up((size_t)B * C * H * W * 4, 256);
  const char* maps = (const char*)scratch + align_up(nblk * 4, 256);
  const int tiles_x = (W + ST - 1) / ST, tiles_y = (H + STY - 1) / STY;
  { ProfScope ps_(KID_SSIM_BWD, stream);
    hipLaunchKernelGGL(ssim_bwd_kernel, dim3((unsigned)nblk), dim3(256), 0, stream, img1, img2, H, W, tiles_x, tiles_y,
                       (const float*)maps,
                       (const float*)(maps + plane), (const float*)(maps + 2 * plane), dL_dmean,
                       1.0f / (float)((double)B * C * H * W), dL_dimg1); }
  SFGS_POST_LAUNCH("ssim_bwd", stream, 0);
  return SFGS_OK;
}
