// importance.hip -- per-Gaussian blend-weight statistics of a rendered view (ABI 28; Python: sfgs/importance.py).
//
// blend_stats_kernel walks the per-tile lists of a finished sfgs_raster_forward_render exactly as composite_fwd_kernel<false>
// (composite_fwd.hip) does -- same tile -> wave mapping, same pixel coordinates, the same eval_splat / pixel_fwd_step per
// (pixel, entry) pair in list order -- and, instead of an image, adds per Gaussian: the sum of the blend weights w = alpha T of
// the pairs that were blended, their number, and the largest w. The forward's strip lists are left out: a pair they skip is a
// pair eval_splat rejects, and a rejected pair leaves the pixel's state as it was, so every decision, T and w are the image's.
//
// Sums are integers (floor(w 2^32), w <= 0.99): exact, independent of the order of the tiles. No float atomics.
// Compile with -ffp-contract=off (raster_math.h).
#include "sfgs_internal.h"

namespace sfgs {

// Sixteen entries at a time: every lane holds its pixel's (q, w) of the sixteen entries, and four exchange steps over a DPP row
// (lane ^ 8, 4, 2, 1) leave lane r of each row with entry r's totals over the row -- 8 + 4 + 2 + 1 = 15 exchanges per quantity instead
// of 16 x 4; two more steps (lane ^ 16, 32) over the rows finish it. Afterwards every lane l holds the totals of entry l & 15.
template <int HALF>
__device__ __forceinline__ void fold_step(unsigned long long (&q)[16], float (&w)[16], int lane) {
  const bool up = (lane & HALF) != 0;
#pragma unroll
  for (int i = 0; i < HALF; ++i) {
    const unsigned long long qk = up ? q[i + HALF] : q[i], qs = up ? q[i] : q[i + HALF];
    const float wk = up ? w[i + HALF] : w[i], ws = up ? w[i] : w[i + HALF];
    q[i] = qk + (unsigned long long)__shfl_xor((long long)qs, HALF);
    w[i] = fmaxf(wk, __shfl_xor(ws, HALF));
  }
}

__global__ void __launch_bounds__(64)
blend_stats_kernel(KFrame kf, int N, int TX8, int TY8, int SX, int SY, const uint2* __restrict__ tile_range,
                   const uint32_t* __restrict__ sorted_id, const float4* __restrict__ rec, unsigned slot_capacity,
                   const unsigned long long* __restrict__ hdr, const unsigned char* __restrict__ pixel_mask,
                   unsigned long long* __restrict__ sum_q32, unsigned long long* __restrict__ hits,
                   unsigned* __restrict__ max_bits) {
  __shared__ float4 stage[64 * 3];
  int sbx, sby, wave, lw;
  if (!composite_wave_role<1>(SX, SY, sbx, sby, wave, lw)) return;
  const int tx = sbx * 2 + (wave & 1), ty = sby * 2 + (wave >> 1);
  const int lane = threadIdx.x & 63;
  if (tx >= TX8 || ty >= TY8 || ty < kf.band0 || ty >= kf.band1) return;
  const int W = kf.W, H = kf.H;
  const int px = tx * 8 + (lane & 7), py = ty * 8 + (lane >> 3);
  const bool inside = px < W && py < H;
  const size_t pix = (size_t)py * W + px;
  const uint2 tr = tile_range[ty * TX8 + tx];
  const unsigned s = min(tr.x, slot_capacity), e = min(tr.x + tr.y, slot_capacity);   // never past the list arrays
  const float bound = __uint_as_float((unsigned)hdr[HDR_SUBPIX_BOUND]);
  float sx = (float)px, sy = (float)py;
  if (kf.subpix && bound != 0.f && inside) { sx += kf.subpix[pix * 2]; sy += kf.subpix[pix * 2 + 1]; }
  // masked pixels composite like any other (their T decides nothing outside the pixel); only what they add is gated
  const bool counted_px = inside && (pixel_mask == nullptr || pixel_mask[pix] != 0);
  PixelFwd ps;
  pixel_fwd_init(ps, inside);
  // the forward's software pipeline: records of batch i + 1 and ids of batch i + 2 are in flight while batch i is walked
  float4 n0 = make_float4(0.f, 0.f, 0.f, 0.f), n1 = n0, n2 = n0;
  unsigned id_cur = 0, id_next = 0;
  if (s + lane < e) {
    id_cur = sorted_id[s + lane];
    n0 = rec[REC_F4 * (size_t)id_cur]; n1 = rec[REC_F4 * (size_t)id_cur + 1]; n2 = rec[REC_F4 * (size_t)id_cur + 2];
  }
  if (s + 64 + lane < e) id_next = sorted_id[s + 64 + lane];
  for (unsigned b = s; b < e; b += 64) {
    if (__ballot(ps.T > 0.f) == 0ull) break;  // every pixel of the tile is saturated
    const unsigned cnt = min(64u, e - b);
    stage[lane * 3] = n0; stage[lane * 3 + 1] = n1; stage[lane * 3 + 2] = n2;
    const unsigned my_id = id_cur;            // entry `lane` of this batch
    id_cur = id_next;
    if (b + 64 + lane < e) {
      n0 = rec[REC_F4 * (size_t)id_next]; n1 = rec[REC_F4 * (size_t)id_next + 1]; n2 = rec[REC_F4 * (size_t)id_next + 2];
    }
    if (b + 128 + lane < e) id_next = sorted_id[b + 128 + lane];
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const unsigned k0 = b - s;
    unsigned long long my_sum = 0ull;   // entry `lane`: totals over the tile's pixels
    unsigned my_hits = 0u;
    float my_max = 0.f;
#pragma unroll 1
    for (unsigned g = 0; g < cnt; g += 16) {
      unsigned long long q[16];
      float w[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        q[i] = 0ull; w[i] = 0.f;
        const unsigned j = g + i;
        if (j < cnt) {   // wave-uniform
          const float4 r0 = stage[j * 3], r1 = stage[j * 3 + 1];
          const float2 r2 = *reinterpret_cast<const float2*>(&stage[j * 3 + 2]);
          const SplatEval ev = eval_splat(r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, sx, sy);
          const float T_before = ps.T;
          const unsigned last_before = ps.last;
          pixel_fwd_step(ps, ev, r2.y, r1.z, r1.w, r2.x, k0 + j);
          // accepted <=> the step moved `last` (to k0 + j + 1, which no earlier entry can have set); then w is the step's own
          // product alpha * T, formed from the same two floats
          const bool counted = ps.last != last_before && counted_px;
          const float wj = counted ? ev.alpha * T_before : 0.f;
          w[i] = wj;
          q[i] = (unsigned long long)(unsigned)(wj * 4294967296.0f);   // w <= 0.99: fits; truncated
          const unsigned long long bm = __ballot(counted);
          if ((unsigned)lane == j) my_hits = (unsigned)__popcll(bm);
        }
      }
      fold_step<8>(q, w, lane); fold_step<4>(q, w, lane); fold_step<2>(q, w, lane); fold_step<1>(q, w, lane);
      unsigned long long qs = q[0];
      float wm = w[0];
      qs += (unsigned long long)__shfl_xor((long long)qs, 16); wm = fmaxf(wm, __shfl_xor(wm, 16));
      qs += (unsigned long long)__shfl_xor((long long)qs, 32); wm = fmaxf(wm, __shfl_xor(wm, 32));
      if ((unsigned)(lane >> 4) == (g >> 4)) { my_sum = qs; my_max = wm; }
      if (__ballot(ps.T > 0.f) == 0ull) break;
    }
    if (my_hits > 0u && my_id < (unsigned)N) {
      atomicAdd(&sum_q32[my_id], my_sum);
      atomicAdd(&hits[my_id], (unsigned long long)my_hits);
      atomicMax(&max_bits[my_id], __float_as_uint(my_max));   // w >= 0: the integer order of the bits is the float order
    }
    __builtin_amdgcn_wave_barrier();
  }
}

__global__ void __launch_bounds__(256)
blend_stats_views_kernel(int N, const unsigned long long* __restrict__ hits, unsigned long long* __restrict__ hits_seen,
                         uint32_t* __restrict__ views) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const unsigned long long h = hits[i];
  if (h != hits_seen[i]) { ++views[i]; hits_seen[i] = h; }
}

}  // namespace sfgs

using namespace sfgs;

extern "C" int sfgs_raster_blend_stats(const SfgsFrame* frame, int32_t N, const void* geom, const void* tiles, const void* bins,
                                       size_t bins_sz, int64_t dup_capacity, int64_t coarse_capacity,
                                       const unsigned char* pixel_mask, const SfgsBlendStats* out, void* stream_) {
  if (int rc = check_frame(frame)) return rc;
  SFGS_REQUIRE(N >= 0, SFGS_E_ARG, "negative Gaussian count");
  SFGS_REQUIRE(geom && tiles && bins && out, SFGS_E_ARG, "NULL argument");
  SFGS_REQUIRE(out->struct_size == sizeof(SfgsBlendStats), SFGS_E_ARG, "SfgsBlendStats.struct_size %u != %zu (ABI mismatch)",
               out->struct_size, sizeof(SfgsBlendStats));
  SFGS_REQUIRE(out->N == N, SFGS_E_ARG, "SfgsBlendStats.N %d != N %d: the tables belong to another scene", out->N, N);
  SFGS_REQUIRE(N == 0 || (out->weight_sum_q32 && out->hits && out->weight_max), SFGS_E_ARG,
               "SfgsBlendStats table pointer is NULL");
  SFGS_REQUIRE(dup_capacity >= 0 && dup_capacity < (1ll << 32) && coarse_capacity >= 0 && coarse_capacity < (1ll << 31),
               SFGS_E_ARG, "bad dup_capacity / coarse_capacity");
  const int W = frame->image_width, H = frame->image_height;
  const int64_t NCB = coarse_bins(W, H);
  SFGS_REQUIRE(bins_sz >= bins_bytes(dup_capacity, NCB, coarse_capacity), SFGS_E_CAPACITY,
               "bins blob: %zu bytes given, %zu needed", bins_sz, bins_bytes(dup_capacity, NCB, coarse_capacity));
  if (N == 0) return SFGS_OK;
  hipStream_t stream = (hipStream_t)stream_;
  const TilesView tv = tiles_view(const_cast<void*>(tiles), W, H, N, nullptr);
  const GeomView gv = geom_view(const_cast<void*>(geom), N);
  const BinsView bv = bins_view(const_cast<void*>(bins), dup_capacity, NCB, coarse_capacity);
  const KFrame kf = make_kframe(frame);
  const int TX8 = tiles8_x(W), TY8 = tiles8_y(H), SX = (TX8 + 1) / 2, SY = (TY8 + 1) / 2;
  hipLaunchKernelGGL(blend_stats_kernel, dim3(composite_grid(SX, SY, 4)), dim3(64), 0, stream, kf, N, TX8, TY8, SX, SY,
                     tv.tile_range, bv.sorted_id, gv.rec, (unsigned)dup_capacity, tv.hdr, pixel_mask, out->weight_sum_q32,
                     out->hits, reinterpret_cast<unsigned*>(out->weight_max));
  SFGS_POST_LAUNCH("blend_stats", stream, frame->debug);
  return SFGS_OK;
}

extern "C" int sfgs_blend_stats_views(int32_t N, const unsigned long long* hits, unsigned long long* hits_seen, uint32_t* views,
                                      void* stream_) {
  SFGS_REQUIRE(N >= 0, SFGS_E_ARG, "negative Gaussian count");
  SFGS_REQUIRE(N == 0 || (hits && hits_seen && views), SFGS_E_ARG, "NULL argument");
  if (N == 0) return SFGS_OK;
  hipStream_t stream = (hipStream_t)stream_;
  hipLaunchKernelGGL(blend_stats_views_kernel, dim3((N + 255) / 256), dim3(256), 0, stream, N, hits, hits_seen, views);
  SFGS_POST_LAUNCH("blend_stats_views", stream, 0);
  return SFGS_OK;
}
