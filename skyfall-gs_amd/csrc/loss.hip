// loss.hip -- the training loss between render() and loss.backward() (reference train.py:205-234, and :760-799 in the
// IDU episode) as three launches forward and two backward:
//   loss = (1 - lambda_dssim) * L1(mask * image, mask * gt_image) + lambda_dssim * (1 - SSIM(mask * image, mask * gt_image))
//        + lambda_depth * (1 - pearson(mask * gt_depth, mask * depth))        with the NaN / Inf scrub of the depth pair.
// loss_photo_fwd / loss_photo_bwd are ssim.hip's two kernels (same tile, same staging, same fma chain per moment: the SSIM
// value is bit-identical to fused_ssim's when the mask is absent or all ones) with the mask multiplied in on the way to LDS
// and the L1 term taken from the staged tiles. loss_depth_fwd / loss_depth_bwd are streaming passes over the depth pair
// with 16-byte accesses; the Pearson moments are raw sums kept in FLOAT64 (one-pass f32 moments of depths around 400 +- 20
// miss r by 6e-5). loss_final reduces every partial in a fixed order (no float atomics: bit-reproducible), writes the
// scalars and leaves the backward's coefficients in the scratch. Nothing here reads a device value on the host.
// SFGS_LOSS_GT_PREMASKED: the target was resampled after its mask product (resample.hip) and is used AS GIVEN -- the factor on
// its way to LDS is 1 instead of the mask (x * 1 = x exactly); with the bit clear the factor is the mask, the same product as ever.
#include "ssim_tile.h"

namespace sfgs {

__constant__ float LOSS_SSIM_W[11] = SSIM_WINDOW_VALUES;   // ssim.hip's window (ssim_tile.h)

enum { MASK_NONE = 0, MASK_SCALAR = 1, MASK_PLANE = 2 };
constexpr int LOSS_HDR_BYTES = 256;   // head of the scratch: the backward's coefficients (doubles, CF_*)
enum { CF_MEAN_A = 0, CF_MEAN_B, CF_INV_NORM, CF_R_OVER_SAA, CF_R_OVER_SBB, CF_CLAMPED, CF_INV_N, CF_COUNT };
// per-block partial sums of the streaming pass (doubles; a block's row is DS_STRIDE wide)
enum { DS_A = 0, DS_B, DS_AA, DS_BB, DS_AB, DS_N, DS_ABS, DS_COUNT, DS_STRIDE = 8 };
// outputs (floats): loss, Ll1, ssim, depth_loss = 1 - r, r -- and the matching incoming gradients of the backward
enum { OUT_LOSS = 0, OUT_L1, OUT_SSIM, OUT_DEPTH, OUT_R, OUT_COUNT };

// the one-element mask is read from device memory (Camera.original_mask is ones((1,1,1)) on the device for a view
// without a mask): a scalar load per workgroup, no host read
__device__ __forceinline__ float scalar_mask(const float* __restrict__ mask, int mask_mode) {
  return mask_mode == MASK_SCALAR ? mask[0] : 1.0f;
}

template <bool PLANE>
__global__ void __launch_bounds__(256)
loss_photo_fwd_kernel(const float* __restrict__ img1, const float* __restrict__ img2, const float* __restrict__ mask,
                      int mask_mode, int gt_premasked, int H, int W, int tiles_x, int tiles_y, float* __restrict__ ssim_partials,
                      float* __restrict__ l1_partials, float* __restrict__ dm_dmu1, float* __restrict__ dm_dsig1,
                      float* __restrict__ dm_dsig12) {
  __shared__ float s1[SINY][SPITCH], s2[SINY][SPITCH];
  __shared__ float hz[5][SINY][ST];
  __shared__ float red[4], red_l1[4];
  const SsimTile T = ssim_tile(tiles_x, tiles_y);
  const size_t poff = (size_t)T.plane * H * W;
  const uint32_t pbytes = (uint32_t)H * (uint32_t)W * 4u;
  const int x0 = T.x0, y0 = T.y0;
  const int tid = threadIdx.x;
  const WindowWeights ww = window_weights(LOSS_SSIM_W);
  const float ms = scalar_mask(mask, mask_mode);
  // staging as in ssim_fwd_kernel (every load in flight before the first LDS write, addresses clamped into the image);
  // the mask plane -- one for the three colour planes -- is a third load per staged element
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const HaloLane hl = halo_lane(lane, x0, W);
  float r1[SROUNDS], r2[SROUNDS], rm[SROUNDS];
  bool yin[SROUNDS];
  const rsrc_t b1 = plane_rsrc(img1 + poff, pbytes), b2 = plane_rsrc(img2 + poff, pbytes);
  const rsrc_t bm = plane_rsrc(PLANE ? mask : img1 + poff, pbytes);
#pragma unroll
  for (int r = 0; r < SROUNDS; ++r) {
    const uint32_t row = halo_row(4 * r + wv, y0, H, W, yin[r]);
    r1[r] = bload(b1, hl.xoff, row);
    r2[r] = bload(b2, hl.xoff, row);
    if (PLANE) rm[r] = bload(bm, hl.xoff, row);
  }
  if (lane < SIN) {
#pragma unroll
    for (int r = 0; r < SROUNDS; ++r) {
      const bool in = hl.xin && yin[r];
      const float m = PLANE ? rm[r] : ms;
      s1[4 * r + wv][lane] = in ? m * r1[r] : 0.f;
      s2[4 * r + wv][lane] = in ? (gt_premasked ? 1.0f : m) * r2[r] : 0.f;
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
  // vertical pass: thread = (column, group of SQV output rows), as in ssim_fwd_kernel
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
  const rsrc_t o1 = plane_rsrc(dm_dmu1 + poff, pbytes), o2 = plane_rsrc(dm_dsig1 + poff, pbytes),
               o3 = plane_rsrc(dm_dsig12 + poff, pbytes);
  const uint32_t vout = (uint32_t)(ly0 * W + lx) * 4u;
  float vsum = 0.f, l1sum = 0.f;
#pragma unroll
  for (int q = 0; q < SQV; ++q) {
    const int gy = y0 + ly0 + q;
    const uint32_t sout = (uint32_t)((y0 + q) * W + x0) * 4u;
    if (gx < W && gy < H && ly0 + q < STY) {
      const float mu1 = mo[0][q], mu2 = mo[1][q], e11 = mo[2][q], e22 = mo[3][q], e12 = mo[4][q];
      const float mu1sq = mu1 * mu1, mu2sq = mu2 * mu2, mu12 = mu1 * mu2;
      const float sg1 = e11 - mu1sq, sg2 = e22 - mu2sq, sg12 = e12 - mu12;
      const float A1 = 2.f * mu12 + SSIM_C1, A2 = 2.f * sg12 + SSIM_C2;
      const float B1 = mu1sq + mu2sq + SSIM_C1, B2 = sg1 + sg2 + SSIM_C2;
      const float inv = 1.0f / (B1 * B2);
      const float val = A1 * A2 * inv;
      vsum += val;
      // the L1 term: this thread owns the pixel; its masked pair is in the staged tiles
      l1sum += fabsf(s1[ly0 + q + SHALO][lx + SHALO] - s2[ly0 + q + SHALO][lx + SHALO]);
      if (dm_dmu1) {
        const float d_sig1 = -val * (B1 * inv);
        const float d_sig12 = 2.f * A1 * inv;
        bstore(2.f * mu2 * A2 * inv - 2.f * mu1 * val * (B2 * inv) - 2.f * mu1 * d_sig1 - mu2 * d_sig12, o1, vout, sout);
        bstore(d_sig1, o2, vout, sout);
        bstore(d_sig12, o3, vout, sout);
      }
    }
  }
  const float bs = block_sum_256(vsum, red);
  const float bl = block_sum_256(l1sum, red_l1);
  if (tid == 0) { ssim_partials[T.index] = bs; l1_partials[T.index] = bl; }
}

// g_image = mask * (w_ssim * (conv0 + 2 x' conv1 + y' conv2) / count + w_l1 * sign(x' - y') / count), x' = mask * image,
// y' = mask * gt_image (gt_premasked: gt_image).
// gin: the incoming gradients of the five outputs (device memory, OUT_*).
template <bool PLANE>
__global__ void __launch_bounds__(256)
loss_photo_bwd_kernel(const float* __restrict__ img1, const float* __restrict__ img2, const float* __restrict__ mask,
                      int mask_mode, int gt_premasked, int H, int W, int tiles_x, int tiles_y, const float* __restrict__ dm_dmu1,
                      const float* __restrict__ dm_dsig1, const float* __restrict__ dm_dsig12,
                      const float* __restrict__ gin, float lambda_dssim, float one_minus_lambda, float inv_count,
                      float* __restrict__ dL_dimg1) {
  __shared__ float s[3][SINY][SPITCH];
  __shared__ float hz[3][SINY][ST];
  const SsimTile T = ssim_tile(tiles_x, tiles_y);
  const size_t poff = (size_t)T.plane * H * W;
  const uint32_t pbytes = (uint32_t)H * (uint32_t)W * 4u;
  const int x0 = T.x0, y0 = T.y0;
  const int tid = threadIdx.x;
  const WindowWeights ww = window_weights(LOSS_SSIM_W);
  const float ms = scalar_mask(mask, mask_mode);
  const float w_l1 = gin[OUT_LOSS] * one_minus_lambda + gin[OUT_L1];
  const float w_ssim = -gin[OUT_LOSS] * lambda_dssim + gin[OUT_SSIM];
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const HaloLane hl = halo_lane(lane, x0, W);
  float r0[SROUNDS], r1[SROUNDS], r2[SROUNDS];
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
  const int lx = tid & (ST - 1), ly0 = (tid / ST) * SQV;
  const int gx = x0 + lx;
  const rsrc_t b1 = plane_rsrc(img1 + poff, pbytes), b2 = plane_rsrc(img2 + poff, pbytes),
               bm = plane_rsrc(PLANE ? mask : img1 + poff, pbytes), og = plane_rsrc(dL_dimg1 + poff, pbytes);
  const uint32_t vout = (uint32_t)(ly0 * W + lx) * 4u;
  float p1[SQV], p2[SQV], pm[SQV];
#pragma unroll
  for (int q = 0; q < SQV; ++q) {
    const bool ok = gx < W && y0 + ly0 + q < H && ly0 + q < STY;
    const uint32_t sout = (uint32_t)((y0 + q) * W + x0) * 4u;
    p1[q] = bload(b1, ok ? vout : 0u, ok ? sout : 0u);
    p2[q] = bload(b2, ok ? vout : 0u, ok ? sout : 0u);
    pm[q] = PLANE ? bload(bm, ok ? vout : 0u, ok ? sout : 0u) : ms;
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
  const float scale = w_ssim * inv_count, scale_l1 = w_l1 * inv_count;
#pragma unroll
  for (int q = 0; q < SQV; ++q) {
    const int gy = y0 + ly0 + q;
    if (gx < W && gy < H && ly0 + q < STY) {
      const float x = pm[q] * p1[q], y = (gt_premasked ? 1.0f : pm[q]) * p2[q], d = x - y;
      const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
      bstore(pm[q] * (scale * (mo[0][q] + 2.f * x * mo[1][q] + y * mo[2][q]) + scale_l1 * sgn), og, vout,
             (uint32_t)((y0 + q) * W + x0) * 4u);
    }
  }
}

// ---- streaming pass over the depth pair ------------------------------------------------------------------------------------
// a = mask * gt, b = mask * depth; a pair with a non-finite member is scrubbed: ZERO = (0, 0), still counted
// (train.py:229-231); DROP = left out, n counted here (train.py:788-790: no boolean gather, no host wait); KEEP = no scrub
// (the pearson_corrcoef drop-in). A thread takes LS_UNROLL vectors of V floats a block-width apart (all loads in flight
// together), keeps its seven sums in float64 and the block reduces them in a fixed order.
constexpr int LS_THREADS = 256, LS_UNROLL = 4;
enum { INVALID_ZERO = 0, INVALID_DROP = 1, INVALID_KEEP = 2 };

template <int V> struct LossVec;
template <> struct LossVec<4> { using type = float4; };
template <> struct LossVec<1> { using type = float; };
template <int V>
__device__ __forceinline__ void loss_vec_load(const float* __restrict__ p, long long i, float (&out)[V]) {
  const typename LossVec<V>::type v = reinterpret_cast<const typename LossVec<V>::type*>(p)[i];
  if constexpr (V == 4) { out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w; } else { out[0] = v; }
}
template <int V>
__device__ __forceinline__ void loss_vec_store(float* __restrict__ p, long long i, const float (&in)[V]) {
  if constexpr (V == 4) reinterpret_cast<float4*>(p)[i] = make_float4(in[0], in[1], in[2], in[3]);
  else p[i] = in[0];
}

struct DepthSums {
  double s[DS_COUNT];
  __device__ __forceinline__ void add(float gt, float d, float m, int invalid, bool exists) {
    float a = m * gt, b = m * d;
    const bool bad = invalid != INVALID_KEEP && !(isfinite(a) && isfinite(b));
    const bool zero = bad || !exists;
    a = zero ? 0.f : a;
    b = zero ? 0.f : b;
    const double da = (double)a, db = (double)b;
    s[DS_A] += da; s[DS_B] += db;
    s[DS_AA] = fma(da, da, s[DS_AA]); s[DS_BB] = fma(db, db, s[DS_BB]); s[DS_AB] = fma(da, db, s[DS_AB]);
    s[DS_N] += (exists && !(bad && invalid == INVALID_DROP)) ? 1.0 : 0.0;
    s[DS_ABS] += fabs(da - db);
  }
};

template <int V>
__global__ void __launch_bounds__(LS_THREADS)
loss_depth_fwd_kernel(const float* __restrict__ gt, const float* __restrict__ depth, const float* __restrict__ mask,
                      int mask_mode, int invalid, long long n, double* __restrict__ partials) {
  __shared__ double sm[LS_THREADS / 64][DS_COUNT];
  const float ms = scalar_mask(mask, mask_mode);
  const bool plane = mask_mode == MASK_PLANE;   // wave-uniform
  const long long nv = n / V;                    // whole vectors (>= 1: the host picks V = 1 otherwise)
  const long long base = (long long)blockIdx.x * (LS_THREADS * LS_UNROLL) + threadIdx.x;
  float g[LS_UNROLL][V], d[LS_UNROLL][V], m[LS_UNROLL][V];
#pragma unroll
  for (int u = 0; u < LS_UNROLL; ++u) {   // clamped index: always a valid address, no load behind a per-lane condition
    const long long i = base + u * LS_THREADS, ic = i < nv ? i : nv - 1;
    loss_vec_load<V>(gt, ic, g[u]);
    loss_vec_load<V>(depth, ic, d[u]);
    if (plane) loss_vec_load<V>(mask, ic, m[u]);
  }
  DepthSums S;
#pragma unroll
  for (int k = 0; k < DS_COUNT; ++k) S.s[k] = 0.0;
#pragma unroll
  for (int u = 0; u < LS_UNROLL; ++u) {
    const bool exists = base + u * LS_THREADS < nv;
#pragma unroll
    for (int j = 0; j < V; ++j) S.add(g[u][j], d[u][j], plane ? m[u][j] : ms, invalid, exists);
  }
  if (V > 1 && blockIdx.x == 0 && threadIdx.x < n - nv * V) {   // the last n % V elements
    const long long i = nv * V + threadIdx.x;
    S.add(gt[i], depth[i], plane ? mask[i] : ms, invalid, true);
  }
#pragma unroll
  for (int k = 0; k < DS_COUNT; ++k) {
    double v = S.s[k];
#pragma unroll
    for (int dlt = 32; dlt >= 1; dlt >>= 1) v += __shfl_xor(v, dlt);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < DS_COUNT) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < LS_THREADS / 64; ++w) t += sm[w][threadIdx.x];
    partials[(size_t)blockIdx.x * DS_STRIDE + threadIdx.x] = t;
  }
}

// Gradient of the streaming terms w.r.t. x (the other member of the pair is y; `swapped` = x is the pair's FIRST member,
// the reference's gt_depth / torchmetrics' preds):
//   Pearson: g_x = mask * w_depth * -((y' - mean_y) / sqrt(S_xx S_yy) - r (x' - mean_x) / S_xx), 0 for scrubbed / dropped
//            pairs and everywhere while the clamp of r is active; w_depth = g_loss * lambda_depth + g_depth_loss - g_r
//   L1 (l1_only; the l1_loss drop-in): g_x = w_l1 * sign(x - y) / n
template <int V>
__global__ void __launch_bounds__(LS_THREADS)
loss_depth_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ mask,
                      int mask_mode, int invalid, int swapped, int l1_only, long long n, const double* __restrict__ coef,
                      const float* __restrict__ gin, float lambda_depth, float* __restrict__ gx) {
  const float ms = scalar_mask(mask, mask_mode);
  const bool plane = mask_mode == MASK_PLANE;
  const double mean_x = coef[swapped ? CF_MEAN_A : CF_MEAN_B], mean_y = coef[swapped ? CF_MEAN_B : CF_MEAN_A];
  const double inv_norm = coef[CF_INV_NORM], r_over_sxx = coef[swapped ? CF_R_OVER_SAA : CF_R_OVER_SBB];
  const bool clamped = coef[CF_CLAMPED] != 0.0;
  const double w_depth = -(double)(gin[OUT_LOSS] * lambda_depth + gin[OUT_DEPTH] - gin[OUT_R]);
  const double w_l1 = (double)gin[OUT_L1] * coef[CF_INV_N];
  const long long nv = n / V;
  const long long base = (long long)blockIdx.x * (LS_THREADS * LS_UNROLL) + threadIdx.x;
  auto grad = [&](float xv, float yv, float m) -> float {
    if (l1_only) {
      const float dd = xv - yv;
      return (float)(w_l1 * (dd > 0.f ? 1.0 : (dd < 0.f ? -1.0 : 0.0)));
    }
    const float a = m * xv, b = m * yv;
    const bool bad = invalid != INVALID_KEEP && !(isfinite(a) && isfinite(b));
    const double gg = w_depth * (((double)b - mean_y) * inv_norm - r_over_sxx * ((double)a - mean_x));
    return (bad || clamped) ? 0.f : m * (float)gg;
  };
  float xs[LS_UNROLL][V], ys[LS_UNROLL][V], m[LS_UNROLL][V];
#pragma unroll
  for (int u = 0; u < LS_UNROLL; ++u) {
    const long long i = base + u * LS_THREADS, ic = i < nv ? i : nv - 1;
    loss_vec_load<V>(x, ic, xs[u]);
    loss_vec_load<V>(y, ic, ys[u]);
    if (plane) loss_vec_load<V>(mask, ic, m[u]);
  }
#pragma unroll
  for (int u = 0; u < LS_UNROLL; ++u) {
    const long long i = base + u * LS_THREADS;
    float o[V];
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = grad(xs[u][j], ys[u][j], plane ? m[u][j] : ms);
    if (i < nv) loss_vec_store<V>(gx, i, o);
  }
  if (V > 1 && blockIdx.x == 0 && threadIdx.x < n - nv * V) {
    const long long i = nv * V + threadIdx.x;
    gx[i] = grad(x[i], y[i], plane ? mask[i] : ms);
  }
}

// ---- finalisation: ONE workgroup, every partial summed in a fixed order -----------------------------------------------------
// (the order of ssim_mean_kernel: strided per-thread sums, xor-shuffle tree, the 16 wave sums in wave order). The nine sums
// -- SSIM, L1 and the streaming pass's seven -- go through the tree together: two barriers in all.
enum { FS_SSIM = 0, FS_L1 = 1, FS_DEPTH = 2, FS_COUNT = FS_DEPTH + DS_COUNT };

__global__ void __launch_bounds__(1024)
loss_final_kernel(const float* __restrict__ ssim_partials, const float* __restrict__ l1_partials, int n_photo,
                  float inv_count, const double* __restrict__ depth_partials, int n_depth, int depth_is_l1,
                  float lambda_dssim, float lambda_depth, double* __restrict__ coef, float* __restrict__ out) {
  __shared__ double sm[16][FS_COUNT], tot[FS_COUNT];
  const int tid = threadIdx.x;
  double acc[FS_COUNT];
#pragma unroll
  for (int k = 0; k < FS_COUNT; ++k) acc[k] = 0.0;
  for (int i = tid; i < n_photo; i += 1024) { acc[FS_SSIM] += (double)ssim_partials[i]; acc[FS_L1] += (double)l1_partials[i]; }
  for (int i = tid; i < n_depth; i += 1024) {
#pragma unroll
    for (int k = 0; k < DS_COUNT; ++k) acc[FS_DEPTH + k] += depth_partials[(size_t)i * DS_STRIDE + k];
  }
#pragma unroll
  for (int k = 0; k < FS_COUNT; ++k) {
    double v = acc[k];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    if ((tid & 63) == 0) sm[tid >> 6][k] = v;
  }
  __syncthreads();
  if (tid < FS_COUNT) {
    double t = 0.0;
    for (int w = 0; w < 16; ++w) t += sm[w][tid];
    tot[tid] = t;
  }
  __syncthreads();
  if (tid != 0) return;
  const double* S = tot + FS_DEPTH;
  double ll1 = 0.0, ssim = 0.0, depth_loss = 0.0, r_out = 0.0;
  if (n_photo > 0) {
    ssim = tot[FS_SSIM] * (double)inv_count;
    ll1 = tot[FS_L1] * (double)inv_count;
  }
  if (n_depth > 0) {
    const double n = S[DS_N];
    // loss_depth_bwd_kernel loads every coefficient, whichever route it takes: the words this route does not use are
    // zeros, not whatever the scratch held
    for (int k = 0; k < CF_COUNT; ++k) coef[k] = 0.0;
    if (depth_is_l1) {
      ll1 = S[DS_ABS] / n;
      coef[CF_INV_N] = 1.0 / n;
    } else {
      // torchmetrics' _pearson_corrcoef_compute for one update: r = S_ab / sqrt(S_aa S_bb) over the CENTRED sums (the
      // (n - 1) factors cancel); 0 / 0 (n = 0, a constant member) is NaN as in torch -- train.py:792 tests for it
      const double ma = S[DS_A] / n, mb = S[DS_B] / n;
      const double saa = S[DS_AA] - S[DS_A] * ma, sbb = S[DS_BB] - S[DS_B] * mb, sab = S[DS_AB] - S[DS_A] * mb;
      const double inv_norm = 1.0 / sqrt(saa * sbb);
      const double r = sab * inv_norm;
      const double rc = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);   // NaN stays NaN
      r_out = rc;
      depth_loss = 1.0 - rc;
      coef[CF_MEAN_A] = ma; coef[CF_MEAN_B] = mb; coef[CF_INV_NORM] = inv_norm;
      coef[CF_R_OVER_SAA] = r / saa; coef[CF_R_OVER_SBB] = r / sbb;
      coef[CF_CLAMPED] = (r > 1.0 || r < -1.0) ? 1.0 : 0.0;
    }
  }
  // the SSIM mean is rounded exactly as ssim_mean_kernel rounds it: bit-identical to fused_ssim
  double loss = 0.0;
  if (n_photo > 0) loss = (1.0 - (double)lambda_dssim) * ll1 + (double)lambda_dssim * (1.0 - ssim);
  if (n_depth > 0 && !depth_is_l1) loss += (double)lambda_depth * depth_loss;
  out[OUT_LOSS] = (float)loss;
  out[OUT_L1] = (float)ll1;
  out[OUT_SSIM] = (float)ssim;
  out[OUT_DEPTH] = (float)depth_loss;
  out[OUT_R] = (float)r_out;
}

}  // namespace sfgs

using namespace sfgs;

namespace {

struct LossPlan {
  int C, H, W, tiles_x, tiles_y, mask_mode, gt_premasked;
  bool photo, depth, l1_stream, with_grad;
  size_t n_photo;         // tiles = partials of the photometric kernels
  long long n_stream;     // elements of the streaming pass
  size_t n_stream_blocks;
  size_t off_ssim, off_l1, off_depth, off_maps, map_bytes, total;
};

inline size_t stream_blocks(long long n, int V) {
  const long long nv = n / V, per = (long long)LS_THREADS * LS_UNROLL;
  return (size_t)((nv + per - 1) / per);
}

// 0 on success; on failure the message is set and the status returned
int loss_plan(const SfgsLossArgs* a, LossPlan* p) {
  SFGS_REQUIRE(a, SFGS_E_ARG, "NULL SfgsLossArgs");
  SFGS_REQUIRE(a->struct_size == sizeof(SfgsLossArgs), SFGS_E_ARG, "SfgsLossArgs.struct_size %u, expected %zu",
               a->struct_size, sizeof(SfgsLossArgs));
  SFGS_REQUIRE((a->terms & ~(SFGS_LOSS_PHOTOMETRIC | SFGS_LOSS_DEPTH | SFGS_LOSS_L1_STREAM | SFGS_LOSS_GT_PREMASKED)) == 0 &&
                   (a->terms & ~SFGS_LOSS_GT_PREMASKED) != 0,
               SFGS_E_ARG, "SfgsLossArgs.terms %d names no term or an unknown one", a->terms);
  SFGS_REQUIRE(!(a->terms & SFGS_LOSS_GT_PREMASKED) || (a->terms & SFGS_LOSS_PHOTOMETRIC), SFGS_E_ARG,
               "SFGS_LOSS_GT_PREMASKED needs SFGS_LOSS_PHOTOMETRIC");
  SFGS_REQUIRE(!((a->terms & SFGS_LOSS_L1_STREAM) && (a->terms != SFGS_LOSS_L1_STREAM)), SFGS_E_ARG,
               "SFGS_LOSS_L1_STREAM stands alone");
  SFGS_REQUIRE(a->C > 0 && a->H > 0 && a->W > 0, SFGS_E_ARG, "bad image shape [%d,%d,%d]", a->C, a->H, a->W);
  SFGS_REQUIRE(a->invalid_mode >= SFGS_LOSS_INVALID_ZERO && a->invalid_mode <= SFGS_LOSS_INVALID_KEEP, SFGS_E_ARG,
               "SfgsLossArgs.invalid_mode %d", a->invalid_mode);
  const long long P = (long long)a->H * a->W;
  SFGS_REQUIRE(a->mask_elems == 0 || a->mask_elems == 1 || a->mask_elems == P, SFGS_E_ARG,
               "SfgsLossArgs.mask_elems %lld is neither 0, 1 nor H * W", (long long)a->mask_elems);
  SFGS_REQUIRE((a->mask_elems == 0) == (a->mask == nullptr), SFGS_E_ARG, "SfgsLossArgs.mask and mask_elems disagree");
  p->C = a->C; p->H = a->H; p->W = a->W;
  p->photo = a->terms & SFGS_LOSS_PHOTOMETRIC; p->depth = a->terms & SFGS_LOSS_DEPTH;
  p->l1_stream = a->terms & SFGS_LOSS_L1_STREAM; p->with_grad = a->with_grad != 0;
  p->gt_premasked = (a->terms & SFGS_LOSS_GT_PREMASKED) ? 1 : 0;
  p->mask_mode = a->mask_elems == 0 ? MASK_NONE : (a->mask_elems == 1 ? MASK_SCALAR : MASK_PLANE);
  p->tiles_x = (a->W + ST - 1) / ST; p->tiles_y = (a->H + STY - 1) / STY;
  p->n_photo = p->photo ? (size_t)a->C * p->tiles_x * p->tiles_y : 0;
  if (p->photo) {
    SFGS_REQUIRE(a->image && a->gt_image, SFGS_E_ARG, "the photometric term needs image and gt_image");
    SFGS_REQUIRE(p->n_photo <= (size_t)INT32_MAX, SFGS_E_UNSUPPORTED, "more than 2^31 - 1 tiles of 32 x 22");
    SFGS_REQUIRE(P < ((long long)1 << 30), SFGS_E_UNSUPPORTED, "an image plane of 2^30 pixels or more");
  }
  p->n_stream = (p->depth || p->l1_stream) ? (p->l1_stream ? (long long)a->C * P : P) : 0;
  if (p->n_stream) {
    SFGS_REQUIRE(a->depth && a->gt_depth, SFGS_E_ARG, "the depth term needs depth and gt_depth");
    SFGS_REQUIRE(!(p->l1_stream && p->mask_mode != MASK_NONE), SFGS_E_ARG, "SFGS_LOSS_L1_STREAM takes no mask");
  }
  // sized for the scalar route (the most blocks); the route is chosen per call from the pointers' alignment
  p->n_stream_blocks = p->n_stream ? stream_blocks(p->n_stream, 1) : 0;
  SFGS_REQUIRE(p->n_stream_blocks <= (size_t)INT32_MAX, SFGS_E_UNSUPPORTED, "more than 2^41 elements");
  size_t off = LOSS_HDR_BYTES;
  p->off_ssim = off; off += align_up(p->n_photo * 4, 256);
  p->off_l1 = off; off += align_up(p->n_photo * 4, 256);
  p->off_depth = off; off += align_up(p->n_stream_blocks * DS_STRIDE * 8, 256);
  p->map_bytes = align_up((size_t)a->C * P * 4, 256);
  p->off_maps = off;
  if (p->photo && p->with_grad) off += 3 * p->map_bytes;
  p->total = off;
  return SFGS_OK;
}

inline bool aligned16(const void* q) { return ((uintptr_t)q & 15u) == 0; }
inline int stream_vec(const LossPlan& p, const void* a, const void* b, const void* mask) {
  return (p.n_stream >= 4 && aligned16(a) && aligned16(b) && (p.mask_mode != MASK_PLANE || aligned16(mask))) ? 4 : 1;
}

}  // namespace

extern "C" size_t sfgs_loss_scratch_bytes(const SfgsLossArgs* args) {
  LossPlan p;
  return loss_plan(args, &p) == SFGS_OK ? p.total : 0;
}

extern "C" int sfgs_loss_forward(const SfgsLossArgs* args, float* out5, void* scratch, size_t scratch_sz, void* stream_) {
  LossPlan p;
  if (const int rc = loss_plan(args, &p)) return rc;
  SFGS_REQUIRE(out5 && scratch, SFGS_E_ARG, "NULL argument");
  SFGS_REQUIRE(scratch_sz >= p.total, SFGS_E_CAPACITY, "loss scratch too small: %zu < %zu", scratch_sz, p.total);
  hipStream_t stream = (hipStream_t)stream_;
  char* sc = (char*)scratch;
  float* ssim_partials = (float*)(sc + p.off_ssim);
  float* l1_partials = (float*)(sc + p.off_l1);
  double* depth_partials = (double*)(sc + p.off_depth);
  const float inv_count = 1.0f / (float)((double)p.C * p.H * p.W);
  if (p.photo) {
    float* m0 = p.with_grad ? (float*)(sc + p.off_maps) : nullptr;
    float* m1 = p.with_grad ? (float*)(sc + p.off_maps + p.map_bytes) : nullptr;
    float* m2 = p.with_grad ? (float*)(sc + p.off_maps + 2 * p.map_bytes) : nullptr;
    ProfScope ps_(KID_LOSS_PHOTO_FWD, stream);
    if (p.mask_mode == MASK_PLANE)
      hipLaunchKernelGGL(loss_photo_fwd_kernel<true>, dim3((unsigned)p.n_photo), dim3(256), 0, stream, args->image,
                         args->gt_image, args->mask, p.mask_mode, p.gt_premasked, p.H, p.W, p.tiles_x, p.tiles_y, ssim_partials, l1_partials,
                         m0, m1, m2);
    else
      hipLaunchKernelGGL(loss_photo_fwd_kernel<false>, dim3((unsigned)p.n_photo), dim3(256), 0, stream, args->image,
                         args->gt_image, args->mask, p.mask_mode, p.gt_premasked, p.H, p.W, p.tiles_x, p.tiles_y, ssim_partials, l1_partials,
                         m0, m1, m2);
  }
  if (p.photo) SFGS_POST_LAUNCH("loss_photo_fwd", stream, 0);
  int n_depth = 0;
  if (p.n_stream) {
    const int V = stream_vec(p, args->gt_depth, args->depth, args->mask);
    n_depth = (int)stream_blocks(p.n_stream, V);
    ProfScope ps_(KID_LOSS_DEPTH_FWD, stream);
    if (V == 4)
      hipLaunchKernelGGL(loss_depth_fwd_kernel<4>, dim3((unsigned)n_depth), dim3(LS_THREADS), 0, stream, args->gt_depth,
                         args->depth, args->mask, p.mask_mode, args->invalid_mode, p.n_stream, depth_partials);
    else
      hipLaunchKernelGGL(loss_depth_fwd_kernel<1>, dim3((unsigned)n_depth), dim3(LS_THREADS), 0, stream, args->gt_depth,
                         args->depth, args->mask, p.mask_mode, args->invalid_mode, p.n_stream, depth_partials);
  }
  if (p.n_stream) SFGS_POST_LAUNCH("loss_depth_fwd", stream, 0);
  { ProfScope ps_(KID_LOSS_FINAL, stream);
    hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(1024), 0, stream, ssim_partials, l1_partials, (int)p.n_photo,
                       inv_count, depth_partials, n_depth, (int)p.l1_stream, args->lambda_dssim, args->lambda_depth,
                       (double*)sc, out5); }
  SFGS_POST_LAUNCH("loss_final", stream, 0);
  return SFGS_OK;
}

extern "C" int sfgs_loss_backward(const SfgsLossArgs* args, const void* scratch, const float* grad_out5, float* g_image,
                                  float* g_depth, float* g_gt_depth, void* stream_) {
  LossPlan p;
  if (const int rc = loss_plan(args, &p)) return rc;
  SFGS_REQUIRE(scratch && grad_out5, SFGS_E_ARG, "NULL argument");
  SFGS_REQUIRE(!g_image || (p.photo && p.with_grad), SFGS_E_ARG, "g_image needs the photometric term of a with_grad forward");
  SFGS_REQUIRE(!(g_depth || g_gt_depth) || p.n_stream, SFGS_E_ARG, "g_depth / g_gt_depth need the depth term");
  hipStream_t stream = (hipStream_t)stream_;
  const char* sc = (const char*)scratch;
  if (g_image) {
    const float* m0 = (const float*)(sc + p.off_maps);
    const float* m1 = (const float*)(sc + p.off_maps + p.map_bytes);
    const float* m2 = (const float*)(sc + p.off_maps + 2 * p.map_bytes);
    const float inv_count = 1.0f / (float)((double)p.C * p.H * p.W);
    const float one_minus = (float)(1.0 - (double)args->lambda_dssim);
    ProfScope ps_(KID_LOSS_PHOTO_BWD, stream);
    if (p.mask_mode == MASK_PLANE)
      hipLaunchKernelGGL(loss_photo_bwd_kernel<true>, dim3((unsigned)p.n_photo), dim3(256), 0, stream, args->image,
                         args->gt_image, args->mask, p.mask_mode, p.gt_premasked, p.H, p.W, p.tiles_x, p.tiles_y, m0, m1, m2, grad_out5,
                         args->lambda_dssim, one_minus, inv_count, g_image);
    else
      hipLaunchKernelGGL(loss_photo_bwd_kernel<false>, dim3((unsigned)p.n_photo), dim3(256), 0, stream, args->image,
                         args->gt_image, args->mask, p.mask_mode, p.gt_premasked, p.H, p.W, p.tiles_x, p.tiles_y, m0, m1, m2, grad_out5,
                         args->lambda_dssim, one_minus, inv_count, g_image);
  }
  if (g_image) SFGS_POST_LAUNCH("loss_photo_bwd", stream, 0);
  for (int swapped = 0; swapped < 2; ++swapped) {
    float* gx = swapped ? g_gt_depth : g_depth;
    if (!gx) continue;
    const float* x = swapped ? args->gt_depth : args->depth;
    const float* y = swapped ? args->depth : args->gt_depth;
    const int V = (stream_vec(p, x, y, args->mask) == 4 && aligned16(gx)) ? 4 : 1;
    const unsigned blocks = (unsigned)stream_blocks(p.n_stream, V);
    { ProfScope ps_(KID_LOSS_DEPTH_BWD, stream);
      if (V == 4)
        hipLaunchKernelGGL(loss_depth_bwd_kernel<4>, dim3(blocks), dim3(LS_THREADS), 0, stream, x, y, args->mask, p.mask_mode,
                           args->invalid_mode, swapped, (int)p.l1_stream, p.n_stream, (const double*)sc, grad_out5,
                           args->lambda_depth, gx);
      else
        hipLaunchKernelGGL(loss_depth_bwd_kernel<1>, dim3(blocks), dim3(LS_THREADS), 0, stream, x, y, args->mask, p.mask_mode,
                           args->invalid_mode, swapped, (int)p.l1_stream, p.n_stream, (const double*)sc, grad_out5,
                           args->lambda_depth, gx); }
    SFGS_POST_LAUNCH("loss_depth_bwd", stream, 0);
  }
  return SFGS_OK;
}
