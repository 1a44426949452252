// metrics.hip -- the evaluation pass of training_report (reference train.py:1064,1075,1090-1091) in two launches per view:
//   image = clamp(render, 0, 1), gt_image = clamp(original_image, 0, 1)
//   l1_loss(image, gt_image) (utils/loss_utils.py:17-18), psnr(image, gt_image) (utils/image_utils.py:17-19: per plane,
//   20 log10(1 / sqrt(mse))) and, next to them, the SSIM of utils/loss_utils.py:33-63.
// metrics_tile is loss.hip's loss_photo_fwd without the mask and without the three derivative maps (same tile, same staging, same
// fma chain per moment, same tile order: the SSIM value is bit-identical to fused_ssim's) with the clamp applied on the way to
// LDS and sum |a - b|, sum (a - b)^2 taken from the staged tiles. metrics_stream is the route without SSIM: a streaming pass
// over the pair with 16-byte loads, per-thread sums in FLOAT64 (a thread adds 16 terms: in float32 that chain alone would
// use up the error the tests allow). metrics_final reduces every partial in float64 in a fixed order (no float atomics:
// bit-reproducible) and writes the row of eight float64. Nothing here reads a device value on the host; no profiler ids.
#include "ssim_tile.h"

#include <math.h>

namespace sfgs {

__constant__ float METRICS_SSIM_W[11] = SSIM_WINDOW_VALUES;   // ssim.hip's window (ssim_tile.h)

// torch.clamp(x, 0, 1): NaN stays NaN. fminf / fmaxf and v_med3_f32 return the bound for a NaN; two compares and two selects keep
// it but cost four VALU instructions per staged element in a VALU-bound kernel (the tile kernel measured 8 % behind
// loss_photo_fwd with them). IEEE 754-2019 maximum / minimum propagate NaN by definition and are one instruction each on
// gfx950 (v_maximum3_f32, v_minimum3_f32).
template <bool CLAMP>
__device__ __forceinline__ float metrics_clamp(float x) {
  if (!CLAMP) return x;
  return __builtin_elementwise_minimum(__builtin_elementwise_maximum(x, 0.f), 1.f);
}

// block_sum_256 (ssim_tile.h) for three values at once: the same xor tree and the same order of the four wave sums per value
// (the SSIM partial keeps fused_ssim's bits), one barrier instead of three
__device__ __forceinline__ void block_sum3_256(float& a, float& b, float& c, float (*smem)[4]) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { a += __shfl_xor(a, d); b += __shfl_xor(b, d); c += __shfl_xor(c, d); }
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) { smem[0][tid >> 6] = a; smem[1][tid >> 6] = b; smem[2][tid >> 6] = c; }
  __syncthreads();
  a = smem[0][0] + smem[0][1] + smem[0][2] + smem[0][3];
  b = smem[1][0] + smem[1][1] + smem[1][2] + smem[1][3];
  c = smem[2][0] + smem[2][1] + smem[2][2] + smem[2][3];
}

template <bool CLAMP>
__global__ void __launch_bounds__(256)
metrics_tile_kernel(const float* __restrict__ img1, const float* __restrict__ img2, int H, int W, int tiles_x, int tiles_y,
                    float* __restrict__ ssim_partials, float* __restrict__ abs_partials, float* __restrict__ sq_partials) {
  __shared__ float s1[SINY][SPITCH], s2[SINY][SPITCH];
  __shared__ float hz[5][SINY][ST];
  __shared__ float red[3][4];
  const SsimTile T = ssim_tile(tiles_x, tiles_y);
  const size_t poff = (size_t)T.plane * H * W;
  const uint32_t pbytes = (uint32_t)H * (uint32_t)W * 4u;
  const int x0 = T.x0, y0 = T.y0;
  const int tid = threadIdx.x;
  const WindowWeights ww = window_weights(METRICS_SSIM_W);
  // staging as in ssim_fwd_kernel: every load in flight before the first LDS write, addresses clamped into the image
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
      s1[4 * r + wv][lane] = in ? metrics_clamp<CLAMP>(r1[r]) : 0.f;
      s2[4 * r + wv][lane] = in ? metrics_clamp<CLAMP>(r2[r]) : 0.f;
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
  float vsum = 0.f, abs_sum = 0.f, sq_sum = 0.f;
#pragma unroll
  for (int q = 0; q < SQV; ++q) {
    const int gy = y0 + ly0 + q;
    if (gx < W && gy < H && ly0 + q < STY) {
      const float mu1 = mo[0][q], mu2 = mo[1][q], e11 = mo[2][q], e22 = mo[3][q], e12 = mo[4][q];
      const float mu1sq = mu1 * mu1, mu2sq = mu2 * mu2, mu12 = mu1 * mu2;
      const float sg1 = e11 - mu1sq, sg2 = e22 - mu2sq, sg12 = e12 - mu12;
      const float A1 = 2.f * mu12 + SSIM_C1, A2 = 2.f * sg12 + SSIM_C2;
      const float B1 = mu1sq + mu2sq + SSIM_C1, B2 = sg1 + sg2 + SSIM_C2;
      const float inv = 1.0f / (B1 * B2);
      vsum += A1 * A2 * inv;
      // this thread owns the pixel; its (clamped) pair is in the staged tiles
      const float d = s1[ly0 + q + SHALO][lx + SHALO] - s2[ly0 + q + SHALO][lx + SHALO];
      abs_sum += fabsf(d);
      sq_sum += d * d;
    }
  }
  block_sum3_256(vsum, abs_sum, sq_sum, red);
  if (tid == 0) { ssim_partials[T.index] = vsum; abs_partials[T.index] = abs_sum; sq_partials[T.index] = sq_sum; }
}

// ---- the route without SSIM: a streaming pass over the pair ----------------------------------------------------------------
// Workgroup (plane, j) of blocks_per_plane per plane: a thread takes MS_UNROLL vectors of V floats a block-width apart (all
// loads in flight together, the index clamped into the plane: no load behind a per-lane condition), forms d = a - b and d * d
// in float32 as the reference does and keeps its two sums in float64; the block reduces them in a fixed order.
constexpr int MS_THREADS = 256, MS_UNROLL = 4;

template <int V> struct MetricsVec;
template <> struct MetricsVec<4> { using type = float4; };
template <> struct MetricsVec<1> { using type = float; };
template <int V>
__device__ __forceinline__ void metrics_vec_load(const float* __restrict__ p, long long i, float (&out)[V]) {
  const typename MetricsVec<V>::type v = reinterpret_cast<const typename MetricsVec<V>::type*>(p)[i];
  if constexpr (V == 4) { out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w; } else { out[0] = v; }
}

template <int V, bool CLAMP>
__global__ void __launch_bounds__(MS_THREADS)
metrics_stream_kernel(const float* __restrict__ a, const float* __restrict__ b, long long plane_elems, int blocks_per_plane,
                      double* __restrict__ partials) {
  __shared__ double sm[MS_THREADS / 64][2];
  const int plane = (int)blockIdx.x / blocks_per_plane, j = (int)blockIdx.x - plane * blocks_per_plane;
  const float* pa = a + (size_t)plane * plane_elems;
  const float* pb = b + (size_t)plane * plane_elems;
  const long long nv = plane_elems / V;   // whole vectors: the host picks V = 4 only when plane_elems % 4 == 0
  const long long base = (long long)j * (MS_THREADS * MS_UNROLL) + threadIdx.x;
  float x[MS_UNROLL][V], y[MS_UNROLL][V];
#pragma unroll
  for (int u = 0; u < MS_UNROLL; ++u) {
    const long long i = base + u * MS_THREADS, ic = i < nv ? i : nv - 1;
    metrics_vec_load<V>(pa, ic, x[u]);
    metrics_vec_load<V>(pb, ic, y[u]);
  }
  double s_abs = 0.0, s_sq = 0.0;
#pragma unroll
  for (int u = 0; u < MS_UNROLL; ++u) {
    const bool exists = base + u * MS_THREADS < nv;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float d = metrics_clamp<CLAMP>(x[u][k]) - metrics_clamp<CLAMP>(y[u][k]);
      const float ad = fabsf(d), dd = d * d;
      s_abs += exists ? (double)ad : 0.0;   // a select, not a product: a NaN behind the plane's end must not count
      s_sq += exists ? (double)dd : 0.0;
    }
  }
#pragma unroll
  for (int dlt = 32; dlt >= 1; dlt >>= 1) { s_abs += __shfl_xor(s_abs, dlt); s_sq += __shfl_xor(s_sq, dlt); }
  if ((threadIdx.x & 63) == 0) { sm[threadIdx.x >> 6][0] = s_abs; sm[threadIdx.x >> 6][1] = s_sq; }
  __syncthreads();
  if (threadIdx.x < 2) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < MS_THREADS / 64; ++w) t += sm[w][threadIdx.x];
    partials[(size_t)blockIdx.x * 2 + threadIdx.x] = t;
  }
}

// ---- finalisation: ONE workgroup, every partial summed in float64 in a fixed order -----------------------------------------
// (the order of ssim_mean_kernel / loss_final_kernel: strided per-thread sums, xor-shuffle tree, the 16 wave sums in wave
// order). n_tile > 0: the tile route's three float arrays; otherwise n_stream blocks of two doubles. Partial i belongs to plane
// i / per_plane on either route (plane-major order).
enum { MF_SSIM = 0, MF_ABS = 1, MF_SQ = 2, MF_COUNT = MF_SQ + 4 };
enum { ROW_L1 = 0, ROW_PSNR, ROW_SSIM, ROW_MSE, ROW_PLANE0 };

__global__ void __launch_bounds__(1024)
metrics_final_kernel(const float* __restrict__ ssim_partials, const float* __restrict__ abs_partials,
                     const float* __restrict__ sq_partials, int n_tile, const double* __restrict__ stream_partials,
                     int n_stream, int per_plane, int P, double plane_elems, float inv_count, int want_ssim, int plane_mse,
                     double* __restrict__ row) {
  __shared__ double sm[16][MF_COUNT], tot[MF_COUNT];
  const int tid = threadIdx.x;
  double acc[MF_COUNT];
#pragma unroll
  for (int k = 0; k < MF_COUNT; ++k) acc[k] = 0.0;
  for (int i = tid; i < n_tile; i += 1024) {
    const int plane = i / per_plane;
    const double q = (double)sq_partials[i];
    acc[MF_SSIM] += (double)ssim_partials[i];
    acc[MF_ABS] += (double)abs_partials[i];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[MF_SQ + c] += plane == c ? q : 0.0;
  }
  for (int i = tid; i < n_stream; i += 1024) {
    const int plane = i / per_plane;
    const double q = stream_partials[(size_t)i * 2 + 1];
    acc[MF_ABS] += stream_partials[(size_t)i * 2];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[MF_SQ + c] += plane == c ? q : 0.0;
  }
#pragma unroll
  for (int k = 0; k < MF_COUNT; ++k) {
    double v = acc[k];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    if ((tid & 63) == 0) sm[tid >> 6][k] = v;
  }
  __syncthreads();
  if (tid < MF_COUNT) {
    double t = 0.0;
    for (int w = 0; w < 16; ++w) t += sm[w][tid];
    tot[tid] = t;
  }
  __syncthreads();
  if (tid != 0) return;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const double count = plane_elems * (double)P;
  double sq_all = 0.0, psnr_sum = 0.0;
  for (int c = 0; c < 4; ++c) {
    double slot = nan;
    if (c < P) {
      const double mse_c = tot[MF_SQ + c] / plane_elems;
      const double psnr_c = 20.0 * log10(1.0 / sqrt(mse_c));   // mse_c = 0: +inf; NaN stays NaN
      sq_all += tot[MF_SQ + c];
      psnr_sum += psnr_c;
      slot = plane_mse ? mse_c : psnr_c;
    }
    row[ROW_PLANE0 + c] = slot;
  }
  row[ROW_L1] = tot[MF_ABS] / count;
  row[ROW_PSNR] = psnr_sum / (double)P;
  // the SSIM mean is formed exactly as ssim_mean_kernel forms it: its float32 rounding is fused_ssim's value
  row[ROW_SSIM] = want_ssim ? tot[MF_SSIM] * (double)inv_count : nan;
  row[ROW_MSE] = sq_all / count;
}

}  // namespace sfgs

using namespace sfgs;

namespace {

struct MetricsPlan {
  int P, H, W, tiles_x, tiles_y;
  bool ssim, clamp, plane_mse;
  long long plane_elems;
  size_t n_tile;               // tiles = partials of the tile route (0 on the stream route)
  size_t stream_blocks_max;    // per plane, sized for the scalar route (the most blocks)
  size_t total;
};

inline size_t metrics_stream_blocks(long long plane_elems, int V) {
  const long long nv = plane_elems / V, per = (long long)MS_THREADS * MS_UNROLL;
  return (size_t)((nv + per - 1) / per);
}

// 0 on success; on failure the message is set and the status returned
int metrics_plan(const SfgsMetricsArgs* a, MetricsPlan* p) {
  SFGS_REQUIRE(a, SFGS_E_ARG, "NULL SfgsMetricsArgs");
  SFGS_REQUIRE(a->struct_size == sizeof(SfgsMetricsArgs), SFGS_E_ARG, "SfgsMetricsArgs.struct_size %u, expected %zu",
               a->struct_size, sizeof(SfgsMetricsArgs));
  SFGS_REQUIRE(a->P >= 1 && a->P <= 4, SFGS_E_ARG, "SfgsMetricsArgs.P %d: 1 to 4 planes", a->P);
  SFGS_REQUIRE(a->H > 0 && a->W > 0, SFGS_E_ARG, "SfgsMetricsArgs: H %d, W %d", a->H, a->W);
  SFGS_REQUIRE((a->flags & ~(SFGS_METRICS_CLAMP | SFGS_METRICS_SSIM | SFGS_METRICS_PLANE_MSE)) == 0, SFGS_E_ARG,
               "SfgsMetricsArgs.flags %d has an unknown bit", a->flags);
  SFGS_REQUIRE(a->a && a->b, SFGS_E_ARG, "SfgsMetricsArgs: a or b is NULL");
  SFGS_REQUIRE((long long)a->H * a->W < (1ll << 30), SFGS_E_UNSUPPORTED, "an image plane of 2^30 pixels or more");
  p->P = a->P; p->H = a->H; p->W = a->W;
  p->clamp = a->flags & SFGS_METRICS_CLAMP; p->ssim = a->flags & SFGS_METRICS_SSIM;
  p->plane_mse = a->flags & SFGS_METRICS_PLANE_MSE;
  p->plane_elems = (long long)a->H * a->W;
  p->tiles_x = (a->W + ST - 1) / ST; p->tiles_y = (a->H + STY - 1) / STY;
  p->n_tile = p->ssim ? (size_t)a->P * p->tiles_x * p->tiles_y : 0;
  SFGS_REQUIRE(p->n_tile <= (size_t)INT32_MAX, SFGS_E_UNSUPPORTED, "more than 2^31 - 1 tiles of 32 x 22");
  p->stream_blocks_max = p->ssim ? 0 : metrics_stream_blocks(p->plane_elems, 1);
  p->total = p->ssim ? 3 * align_up(p->n_tile * 4, 256) : align_up((size_t)a->P * p->stream_blocks_max * 16, 256);
  return SFGS_OK;
}

inline bool metrics_aligned16(const void* q) { return ((uintptr_t)q & 15u) == 0; }

}  // namespace

extern "C" size_t sfgs_metrics_scratch_bytes(const SfgsMetricsArgs* args) {
  MetricsPlan p;
  return metrics_plan(args, &p) == SFGS_OK ? p.total : 0;
}

extern "C" int sfgs_metrics_view(const SfgsMetricsArgs* args, double* row8, void* scratch, size_t scratch_bytes,
                                 void* stream_) {
  MetricsPlan p;
  if (const int rc = metrics_plan(args, &p)) return rc;
  SFGS_REQUIRE(row8 && scratch, SFGS_E_ARG, "NULL argument");
  SFGS_REQUIRE(scratch_bytes >= p.total, SFGS_E_CAPACITY, "metrics scratch too small: %zu < %zu", scratch_bytes, p.total);
  hipStream_t stream = (hipStream_t)stream_;
  char* sc = (char*)scratch;
  const float inv_count = 1.0f / (float)((double)p.P * p.H * p.W);   // as sfgs_ssim_forward forms it
  if (p.ssim) {
    const size_t stride = align_up(p.n_tile * 4, 256);
    float* ssim_partials = (float*)sc;
    float* abs_partials = (float*)(sc + stride);
    float* sq_partials = (float*)(sc + 2 * stride);
    if (p.clamp)
      hipLaunchKernelGGL(metrics_tile_kernel<true>, dim3((unsigned)p.n_tile), dim3(256), 0, stream, args->a, args->b, p.H, p.W,
                         p.tiles_x, p.tiles_y, ssim_partials, abs_partials, sq_partials);
    else
      hipLaunchKernelGGL(metrics_tile_kernel<false>, dim3((unsigned)p.n_tile), dim3(256), 0, stream, args->a, args->b, p.H, p.W,
                         p.tiles_x, p.tiles_y, ssim_partials, abs_partials, sq_partials);
    SFGS_POST_LAUNCH("metrics_tile", stream, 0);
    hipLaunchKernelGGL(metrics_final_kernel, dim3(1), dim3(1024), 0, stream, (const float*)ssim_partials,
                       (const float*)abs_partials, (const float*)sq_partials, (int)p.n_tile, (const double*)nullptr, 0,
                       p.tiles_x * p.tiles_y, p.P, (double)p.plane_elems, inv_count, 1, (int)p.plane_mse, row8);
  } else {
    const int V = (p.plane_elems % 4 == 0 && metrics_aligned16(args->a) && metrics_aligned16(args->b)) ? 4 : 1;
    const int bpp = (int)metrics_stream_blocks(p.plane_elems, V);
    const dim3 grid((unsigned)(p.P * bpp)), block(MS_THREADS);
    double* partials = (double*)sc;
    if (V == 4) {
      if (p.clamp) hipLaunchKernelGGL((metrics_stream_kernel<4, true>), grid, block, 0, stream, args->a, args->b, p.plane_elems, bpp, partials);
      else hipLaunchKernelGGL((metrics_stream_kernel<4, false>), grid, block, 0, stream, args->a, args->b, p.plane_elems, bpp, partials);
    } else {
      if (p.clamp) hipLaunchKernelGGL((metrics_stream_kernel<1, true>), grid, block, 0, stream, args->a, args->b, p.plane_elems, bpp, partials);
      else hipLaunchKernelGGL((metrics_stream_kernel<1, false>), grid, block, 0, stream, args->a, args->b, p.plane_elems, bpp, partials);
    }
    SFGS_POST_LAUNCH("metrics_stream", stream, 0);
    hipLaunchKernelGGL(metrics_final_kernel, dim3(1), dim3(1024), 0, stream, (const float*)nullptr, (const float*)nullptr,
                       (const float*)nullptr, 0, (const double*)partials, p.P * bpp, bpp, p.P, (double)p.plane_elems, inv_count,
                       0, (int)p.plane_mse, row8);
  }
  SFGS_POST_LAUNCH("metrics_final", stream, 0);
  return SFGS_OK;
}
