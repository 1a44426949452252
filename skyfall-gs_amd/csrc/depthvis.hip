// depthvis.hip -- colorize_depth_torch (reference render_video.py:129-170; the same function in render_video_from_ply.py:126-167
// and train.py:1001-1041) on the device, bit for bit (include/sfgs.h spells the float32 sequence):
//     disp = 1 / depth on the valid pixels (depth > 0, and the mask), lo / hi = numpy's nanquantile(disp, 0.01 / 0.99),
//     x = 1 - (disp - lo) / (hi - lo), colour = lut[index(x * 256)], black for NaN
// and the frame quantiser of render_video.py:264.
// The two quantiles need the order statistics i and i + 1 each: four ranks, found EXACTLY by a radix select over the
// disparity's bit pattern (a valid disparity is >= +0, so its uint32 pattern orders like its value): three histogram passes
// over the frame (bits 31..21, 20..10, 9..0), each followed by a one-workgroup scan that turns every rank into a bin and a
// rank inside that bin. Passes 2 and 3 count only the pixels whose upper bits equal a prefix found so far; the four ranks
// share at most four distinct prefixes ("slots": ranks with the same prefix share one histogram).
// depthvis_hist<PASS>: up to 256 workgroups of 1024 threads, 4 pixels per thread and step, a histogram per slot in LDS (integer
// LDS atomics), the non-zero bins flushed with integer global atomics: sums of integers, so the result is the same whatever
// the arrival order. No float atomics. depthvis_scan<PASS>: block scan of every slot's histogram; the last one forms lo and hi.
// depthvis_color: 4 pixels per thread, the table in LDS (as k / 255 for the float output).
// Launches of a whole call: memset + 3 + 3 + 1 = 8 (normalize off: 1). The kernels have no profiler ids (the id list of
// sfgs_profile_kernel_name is closed by the loss kernels); tools/bench_depthvis.py takes their times from torch.profiler.
#include "sfgs_internal.h"

#include <math.h>

namespace sfgs {

constexpr int DV_THREADS = 1024;       // histogram and scan kernels
constexpr int DV_MAX_BLOCKS = 256;     // every workgroup flushes up to 4 x 2048 bins: few, large workgroups bound the global atomics
                                       // (a choice for that bound; not compared with more, smaller workgroups)
constexpr int DV_PIX = 4;              // pixels per thread and step
constexpr int DV_BINS1 = 2048, DV_BINS2 = 2048, DV_BINS3 = 1024;   // 11 + 11 + 10 bits
constexpr int DV_SLOTS = 4;
constexpr int DV_COLOR_THREADS = 256;
constexpr int DV_COLOR_MAX_BLOCKS = 2048;

struct DvState {               // head of the scratch (256 bytes reserved)
  uint32_t n;                  // valid pixels
  uint32_t k[4];               // per rank: the rank inside the pixels that carry `prefix`
  uint32_t prefix[4];          // per rank: the upper bits found so far
  uint32_t slot[4];            // per rank: its histogram of the next pass
  uint32_t nslots;             // distinct prefixes (0 when n == 0)
  uint32_t slot_prefix[4];
  float g[2];                  // the two interpolation weights
  float lo, hi;
};
static_assert(sizeof(DvState) <= 256, "DvState");

template <int PASS> struct DvPass;
template <> struct DvPass<1> { static constexpr int BINS = DV_BINS1, SLOTS = 1, BITS = 11; };
template <> struct DvPass<2> { static constexpr int BINS = DV_BINS2, SLOTS = DV_SLOTS, BITS = 11; };
template <> struct DvPass<3> { static constexpr int BINS = DV_BINS3, SLOTS = DV_SLOTS, BITS = 10; };

constexpr size_t DV_OFF_H1 = 256;
constexpr size_t DV_OFF_H2 = DV_OFF_H1 + (size_t)DV_BINS1 * 4;
constexpr size_t DV_OFF_H3 = DV_OFF_H2 + (size_t)DV_SLOTS * DV_BINS2 * 4;
constexpr size_t DV_SCRATCH = DV_OFF_H3 + (size_t)DV_SLOTS * DV_BINS3 * 4;
static_assert(DV_SCRATCH % 16 == 0, "the memset clears whole 16-byte blocks");

// pixels 4 g .. 4 g + 3: the depth where the pixel exists and is valid (> 0, and the mask), else 0 (which is not valid)
template <bool VEC>
__device__ __forceinline__ void dv_load(const float* __restrict__ depth, const unsigned char* __restrict__ mask, long long g,
                                        long long P, float (&d)[DV_PIX]) {
  const long long p0 = g * DV_PIX;
  if (VEC) {   // P % 4 == 0 and aligned pointers: the group is whole
    const float4 v = reinterpret_cast<const float4*>(depth)[g];
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    if (mask) {
      const uint32_t m = reinterpret_cast<const uint32_t*>(mask)[g];
#pragma unroll
      for (int j = 0; j < DV_PIX; ++j) if (((m >> (8 * j)) & 0xffu) == 0) d[j] = 0.f;
    }
  } else {
#pragma unroll
    for (int j = 0; j < DV_PIX; ++j) {
      const long long p = p0 + j;
      d[j] = 0.f;
      if (p < P && (!mask || mask[p] != 0)) d[j] = depth[p];
    }
  }
#pragma unroll
  for (int j = 0; j < DV_PIX; ++j) if (!(d[j] > 0.f)) d[j] = 0.f;   // NaN, <= 0
}

template <int PASS, bool VEC>
__global__ void __launch_bounds__(DV_THREADS)
depthvis_hist_kernel(const float* __restrict__ depth, const unsigned char* __restrict__ mask, long long P,
                     const DvState* __restrict__ st, uint32_t* __restrict__ hist) {
  constexpr int BINS = DvPass<PASS>::BINS;
  __shared__ uint32_t sh[DvPass<PASS>::SLOTS * BINS];
  uint32_t nslots = 1, sp[DV_SLOTS] = {0, 0, 0, 0};
  if (PASS > 1) {
    nslots = st->nslots < (uint32_t)DV_SLOTS ? st->nslots : (uint32_t)DV_SLOTS;
#pragma unroll
    for (int s = 0; s < DV_SLOTS; ++s) sp[s] = st->slot_prefix[s];
    if (nslots == 0) return;   // no valid pixel
  }
  const uint32_t used = nslots * BINS;
  for (uint32_t i = threadIdx.x; i < used; i += DV_THREADS) sh[i] = 0;
  __syncthreads();
  const long long groups = (P + DV_PIX - 1) / DV_PIX, stride = (long long)gridDim.x * DV_THREADS;
  for (long long g = (long long)blockIdx.x * DV_THREADS + threadIdx.x; g < groups; g += stride) {
    float d[DV_PIX];
    dv_load<VEC>(depth, mask, g, P, d);
#pragma unroll
    for (int j = 0; j < DV_PIX; ++j) {
      if (!(d[j] > 0.f)) continue;
      const uint32_t key = __float_as_uint(1.0f / d[j]);   // <= 0x7f800000
      if (PASS == 1) {
        atomicAdd(&sh[key >> 21], 1u);
      } else {
        const uint32_t upper = PASS == 2 ? key >> 21 : key >> 10;
        const uint32_t bin = PASS == 2 ? (key >> 10) & 2047u : key & 1023u;
#pragma unroll
        for (int s = 0; s < DV_SLOTS; ++s)
          if ((uint32_t)s < nslots && upper == sp[s]) atomicAdd(&sh[s * BINS + bin], 1u);
      }
    }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < used; i += DV_THREADS) {
    const uint32_t c = sh[i];
    if (c) atomicAdd(&hist[i], c);
  }
}

// numpy's _lerp on float32 operands
__device__ __forceinline__ float dv_lerp(float a, float b, float g) {
  const float d = b - a;
  float r = a + d * g;
  if (g >= 0.5f) r = b - d * (1.0f - g);
  return r;
}

// ONE workgroup. Pass 1: n and the four ranks from the first histogram; every pass: rank -> (bin, rank inside the bin);
// passes 1 and 2: the slots of the next pass; pass 3: the four values, lo and hi.
template <int PASS>
__global__ void __launch_bounds__(DV_THREADS)
depthvis_scan_kernel(DvState* __restrict__ st, const uint32_t* __restrict__ hist) {
  constexpr int BINS = DvPass<PASS>::BINS, PER = BINS / DV_THREADS, BITS = DvPass<PASS>::BITS;
  __shared__ unsigned smem[DV_THREADS / 64 + 1];
  __shared__ uint32_t found_bin[4], found_excl[4];
  const unsigned tid = threadIdx.x;
  uint32_t k[4] = {0, 0, 0, 0}, slot[4] = {0, 0, 0, 0}, nslots = 1, n = 0;
  float gq[2] = {0.f, 0.f};
  if (PASS > 1) {
    nslots = st->nslots < (uint32_t)DV_SLOTS ? st->nslots : (uint32_t)DV_SLOTS;
#pragma unroll
    for (int r = 0; r < 4; ++r) { k[r] = st->k[r]; slot[r] = st->slot[r] & 3u; }
  }
  if (tid < 4) { found_bin[tid] = 0; found_excl[tid] = 0; }   // a rank that no bin holds (n == 0) stays in range
  for (uint32_t s = 0; s < nslots; ++s) {
    uint32_t c[PER], sum = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) { c[j] = hist[s * BINS + tid * PER + j]; sum += c[j]; }
    unsigned total;
    const unsigned excl = block_excl_scan_u32<DV_THREADS>(sum, &total, smem);
    if (PASS == 1) {
      n = total;
      if (n > 0) {
        const float nm1 = (float)(n - 1);
        const float q[2] = {0.01f, 0.99f};
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const float vi = nm1 * q[j];
          const float fl = floorf(vi);
          const uint32_t i = (uint32_t)fl;
          gq[j] = vi - fl;
          k[2 * j] = i;
          k[2 * j + 1] = i + 1 < n ? i + 1 : n - 1;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (slot[r] != s) continue;
      uint32_t run = excl;
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        if (k[r] >= run && k[r] - run < c[j]) { found_bin[r] = tid * PER + j; found_excl[r] = run; }
        run += c[j];
      }
    }
  }
  __syncthreads();
  if (tid != 0) return;
  uint32_t prefix[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    prefix[r] = ((PASS == 1 ? 0u : st->prefix[r]) << BITS) | found_bin[r];
    st->prefix[r] = prefix[r];
    st->k[r] = k[r] - found_excl[r];
  }
  if (PASS == 1) { st->n = n; st->g[0] = gq[0]; st->g[1] = gq[1]; }
  if (PASS < 3) {
    uint32_t ns = 0, sps[4] = {0, 0, 0, 0};
    for (int r = 0; r < 4; ++r) {
      uint32_t s = ns;
      for (uint32_t t = 0; t < ns; ++t) if (sps[t] == prefix[r]) { s = t; break; }
      if (s == ns) sps[ns++] = prefix[r];
      st->slot[r] = s;
    }
    for (int s = 0; s < 4; ++s) st->slot_prefix[s] = sps[s];
    const uint32_t n_all = PASS == 1 ? n : st->n;
    st->nslots = n_all > 0 ? ns : 0;
  } else {
    const float nan = __uint_as_float(0x7fc00000u);
    const bool any = st->n > 0;
    st->lo = any ? dv_lerp(__uint_as_float(prefix[0]), __uint_as_float(prefix[1]), st->g[0]) : nan;
    st->hi = any ? dv_lerp(__uint_as_float(prefix[2]), __uint_as_float(prefix[3]), st->g[1]) : nan;
  }
}

// colour index of x (matplotlib's Colormap.__call__ on a float32 array with N = 256); -1: NaN, the "bad" colour (0, 0, 0)
__device__ __forceinline__ int dv_index(float x) {
  if (x != x) return -1;
  const float t = x * 256.0f;
  if (t == 256.0f) return 255;
  if (t < 0.f) return 0;
  if (t >= 256.0f) return 255;
  return (int)t;
}

template <bool U8, bool VEC>
__global__ void __launch_bounds__(DV_COLOR_THREADS)
depthvis_color_kernel(const float* __restrict__ depth, const unsigned char* __restrict__ mask, long long P,
                      const unsigned char* __restrict__ lut, const DvState* __restrict__ st, void* __restrict__ out_) {
  __shared__ float lutf[768];          // float output: k / 255
  __shared__ unsigned char lutb[768];
  for (int i = threadIdx.x; i < 768; i += DV_COLOR_THREADS) {
    const unsigned char v = lut[i];
    if (U8) lutb[i] = v; else lutf[i] = (float)v / 255.0f;
  }
  float lo = 0.f, hi = 1.f;            // normalize off: x = 1 - (disp - 0) / (1 - 0) = 1 - disp, the same bits
  if (st) { lo = st->lo; hi = st->hi; }
  __syncthreads();
  const float span = hi - lo;
  const long long groups = (P + DV_PIX - 1) / DV_PIX, stride = (long long)gridDim.x * DV_COLOR_THREADS;
  for (long long g = (long long)blockIdx.x * DV_COLOR_THREADS + threadIdx.x; g < groups; g += stride) {
    float d[DV_PIX];
    dv_load<VEC>(depth, mask, g, P, d);
    int k[DV_PIX];
#pragma unroll
    for (int j = 0; j < DV_PIX; ++j) {
      k[j] = -1;
      if (d[j] > 0.f) {
        const float disp = 1.0f / d[j];
        k[j] = dv_index(1.0f - (disp - lo) / span);
      }
    }
    const long long p0 = g * DV_PIX;
    if (U8) {
      unsigned char b[3 * DV_PIX];
#pragma unroll
      for (int j = 0; j < DV_PIX; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) b[3 * j + c] = k[j] < 0 ? (unsigned char)0 : lutb[3 * k[j] + c];
      unsigned char* out = (unsigned char*)out_;
      if (VEC) {
        uint32_t* o = reinterpret_cast<uint32_t*>(out) + 3 * g;
#pragma unroll
        for (int w = 0; w < 3; ++w)
          o[w] = (uint32_t)b[4 * w] | (uint32_t)b[4 * w + 1] << 8 | (uint32_t)b[4 * w + 2] << 16 | (uint32_t)b[4 * w + 3] << 24;
      } else {
#pragma unroll
        for (int j = 0; j < DV_PIX; ++j)
          if (p0 + j < P) {
#pragma unroll
            for (int c = 0; c < 3; ++c) out[3 * (p0 + j) + c] = b[3 * j + c];
          }
      }
    } else {
      float* out = (float*)out_;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float v[DV_PIX];
#pragma unroll
        for (int j = 0; j < DV_PIX; ++j) v[j] = k[j] < 0 ? 0.f : lutf[3 * k[j] + c];
        if (VEC) {
          reinterpret_cast<float4*>(out + (long long)c * P)[g] = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
          for (int j = 0; j < DV_PIX; ++j) if (p0 + j < P) out[(long long)c * P + p0 + j] = v[j];
        }
      }
    }
  }
}

// fq_byte, the quantiser itself: sfgs_internal.h (pointcloud.hip colours its rows with it)
template <bool VEC>
__global__ void __launch_bounds__(DV_COLOR_THREADS)
frame_quantize_kernel(const float* __restrict__ image, long long P, unsigned char* __restrict__ out) {
  const long long groups = (P + DV_PIX - 1) / DV_PIX, stride = (long long)gridDim.x * DV_COLOR_THREADS;
  for (long long g = (long long)blockIdx.x * DV_COLOR_THREADS + threadIdx.x; g < groups; g += stride) {
    const long long p0 = g * DV_PIX;
    unsigned char b[3 * DV_PIX];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v[DV_PIX] = {0.f, 0.f, 0.f, 0.f};
      if (VEC) {
        const float4 q = reinterpret_cast<const float4*>(image + (long long)c * P)[g];
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
      } else {
#pragma unroll
        for (int j = 0; j < DV_PIX; ++j) if (p0 + j < P) v[j] = image[(long long)c * P + p0 + j];
      }
#pragma unroll
      for (int j = 0; j < DV_PIX; ++j) b[3 * j + c] = fq_byte(v[j]);
    }
    if (VEC) {
      uint32_t* o = reinterpret_cast<uint32_t*>(out) + 3 * g;
#pragma unroll
      for (int w = 0; w < 3; ++w)
        o[w] = (uint32_t)b[4 * w] | (uint32_t)b[4 * w + 1] << 8 | (uint32_t)b[4 * w + 2] << 16 | (uint32_t)b[4 * w + 3] << 24;
    } else {
#pragma unroll
      for (int j = 0; j < DV_PIX; ++j)
        if (p0 + j < P) {
#pragma unroll
          for (int c = 0; c < 3; ++c) out[3 * (p0 + j) + c] = b[3 * j + c];
        }
    }
  }
}

}  // namespace sfgs

using namespace sfgs;

namespace {

struct DvPlan {
  long long P;
  int hist_blocks, color_blocks;
};

int dv_plan(const SfgsDepthVisArgs* a, DvPlan* p) {
  SFGS_REQUIRE(a, SFGS_E_ARG, "NULL SfgsDepthVisArgs");
  SFGS_REQUIRE(a->struct_size == sizeof(SfgsDepthVisArgs), SFGS_E_ARG, "SfgsDepthVisArgs.struct_size %u, expected %zu",
               a->struct_size, sizeof(SfgsDepthVisArgs));
  SFGS_REQUIRE(a->H > 0 && a->W > 0, SFGS_E_ARG, "SfgsDepthVisArgs: H %d, W %d", a->H, a->W);
  SFGS_REQUIRE((long long)a->H * a->W <= (1ll << 30), SFGS_E_UNSUPPORTED, "SfgsDepthVisArgs: H * W must not exceed 2^30, got %d x %d",
               a->H, a->W);
  SFGS_REQUIRE(a->depth && a->lut, SFGS_E_ARG, "SfgsDepthVisArgs: depth or lut is NULL");
  SFGS_REQUIRE(a->out_kind == SFGS_DEPTHVIS_FLOAT_CHW || a->out_kind == SFGS_DEPTHVIS_UINT8_HWC, SFGS_E_ARG,
               "SfgsDepthVisArgs.out_kind %d", a->out_kind);
  p->P = (long long)a->H * a->W;
  const long long groups = (p->P + DV_PIX - 1) / DV_PIX;
  const long long hb = (groups + DV_THREADS - 1) / DV_THREADS, cb = (groups + DV_COLOR_THREADS - 1) / DV_COLOR_THREADS;
  p->hist_blocks = (int)(hb < DV_MAX_BLOCKS ? hb : DV_MAX_BLOCKS);
  p->color_blocks = (int)(cb < DV_COLOR_MAX_BLOCKS ? cb : DV_COLOR_MAX_BLOCKS);
  return SFGS_OK;
}

inline bool dv_aligned(const void* q, uintptr_t a) { return ((uintptr_t)q & (a - 1)) == 0; }

template <int PASS>
void dv_launch_hist(bool vec, int blocks, hipStream_t stream, const SfgsDepthVisArgs* a, long long P, const DvState* st,
                    uint32_t* hist) {
  if (vec)
    hipLaunchKernelGGL((depthvis_hist_kernel<PASS, true>), dim3((unsigned)blocks), dim3(DV_THREADS), 0, stream, a->depth,
                       a->mask, P, st, hist);
  else
    hipLaunchKernelGGL((depthvis_hist_kernel<PASS, false>), dim3((unsigned)blocks), dim3(DV_THREADS), 0, stream, a->depth,
                       a->mask, P, st, hist);
}

}  // namespace

extern "C" size_t sfgs_depthvis_scratch_bytes(const SfgsDepthVisArgs* args) {
  DvPlan p;
  return dv_plan(args, &p) == SFGS_OK ? DV_SCRATCH : 0;
}

extern "C" int sfgs_depthvis_forward(const SfgsDepthVisArgs* args, void* out, void* scratch, size_t scratch_bytes,
                                     void* stream_) {
  DvPlan p;
  if (const int rc = dv_plan(args, &p)) return rc;
  SFGS_REQUIRE(out, SFGS_E_ARG, "NULL argument");
  const bool normalize = args->normalize != 0;
  if (normalize) {
    SFGS_REQUIRE(scratch, SFGS_E_ARG, "NULL argument");
    SFGS_REQUIRE(scratch_bytes >= DV_SCRATCH, SFGS_E_CAPACITY, "depthvis scratch too small: %zu < %zu", scratch_bytes,
                 DV_SCRATCH);
  }
  hipStream_t stream = (hipStream_t)stream_;
  char* base = (char*)scratch;
  DvState* st = (DvState*)base;
  uint32_t* h1 = (uint32_t*)(base + DV_OFF_H1);
  uint32_t* h2 = (uint32_t*)(base + DV_OFF_H2);
  uint32_t* h3 = (uint32_t*)(base + DV_OFF_H3);
  const bool in_vec = p.P % DV_PIX == 0 && dv_aligned(args->depth, 16) && (!args->mask || dv_aligned(args->mask, 4));
  if (normalize) {
    SFGS_CHECK_HIP(hipMemsetAsync(scratch, 0, DV_SCRATCH, stream));
    dv_launch_hist<1>(in_vec, p.hist_blocks, stream, args, p.P, st, h1);
    SFGS_POST_LAUNCH("depthvis_hist1", stream, 0);
    hipLaunchKernelGGL(depthvis_scan_kernel<1>, dim3(1), dim3(DV_THREADS), 0, stream, st, (const uint32_t*)h1);
    SFGS_POST_LAUNCH("depthvis_scan1", stream, 0);
    dv_launch_hist<2>(in_vec, p.hist_blocks, stream, args, p.P, st, h2);
    SFGS_POST_LAUNCH("depthvis_hist2", stream, 0);
    hipLaunchKernelGGL(depthvis_scan_kernel<2>, dim3(1), dim3(DV_THREADS), 0, stream, st, (const uint32_t*)h2);
    SFGS_POST_LAUNCH("depthvis_scan2", stream, 0);
    dv_launch_hist<3>(in_vec, p.hist_blocks, stream, args, p.P, st, h3);
    SFGS_POST_LAUNCH("depthvis_hist3", stream, 0);
    hipLaunchKernelGGL(depthvis_scan_kernel<3>, dim3(1), dim3(DV_THREADS), 0, stream, st, (const uint32_t*)h3);
    SFGS_POST_LAUNCH("depthvis_scan3", stream, 0);
  }
  const bool u8 = args->out_kind == SFGS_DEPTHVIS_UINT8_HWC;
  const bool vec = in_vec && dv_aligned(out, u8 ? 4 : 16);
  const DvState* cst = normalize ? st : nullptr;
  const dim3 grid((unsigned)p.color_blocks), block(DV_COLOR_THREADS);
  if (u8) {
    if (vec) hipLaunchKernelGGL((depthvis_color_kernel<true, true>), grid, block, 0, stream, args->depth, args->mask, p.P, args->lut, cst, out);
    else hipLaunchKernelGGL((depthvis_color_kernel<true, false>), grid, block, 0, stream, args->depth, args->mask, p.P, args->lut, cst, out);
  } else {
    if (vec) hipLaunchKernelGGL((depthvis_color_kernel<false, true>), grid, block, 0, stream, args->depth, args->mask, p.P, args->lut, cst, out);
    else hipLaunchKernelGGL((depthvis_color_kernel<false, false>), grid, block, 0, stream, args->depth, args->mask, p.P, args->lut, cst, out);
  }
  SFGS_POST_LAUNCH("depthvis_color", stream, 0);
  return SFGS_OK;
}

extern "C" int sfgs_frame_quantize(const float* image, int32_t H, int32_t W, unsigned char* out, void* stream_) {
  SFGS_REQUIRE(H > 0 && W > 0, SFGS_E_ARG, "sfgs_frame_quantize: H %d, W %d", H, W);
  SFGS_REQUIRE((long long)H * W <= (1ll << 30), SFGS_E_UNSUPPORTED, "sfgs_frame_quantize: H * W must not exceed 2^30, got %d x %d", H, W);
  SFGS_REQUIRE(image && out, SFGS_E_ARG, "NULL argument");
  hipStream_t stream = (hipStream_t)stream_;
  const long long P = (long long)H * W, groups = (P + DV_PIX - 1) / DV_PIX;
  const long long cb = (groups + DV_COLOR_THREADS - 1) / DV_COLOR_THREADS;
  const dim3 grid((unsigned)(cb < DV_COLOR_MAX_BLOCKS ? cb : DV_COLOR_MAX_BLOCKS)), block(DV_COLOR_THREADS);
  if (P % DV_PIX == 0 && dv_aligned(image, 16) && dv_aligned(out, 4))
    hipLaunchKernelGGL(frame_quantize_kernel<true>, grid, block, 0, stream, image, P, out);
  else
    hipLaunchKernelGGL(frame_quantize_kernel<false>, grid, block, 0, stream, image, P, out);
  SFGS_POST_LAUNCH("frame_quantize", stream, 0);
  return SFGS_OK;
}
