// opacity_reg.hip -- the opacity-entropy regulariser (reference train.py:236-242, and :834-843 in the IDU episode)
//     opacity = gaussians.get_opacity.clamp(1.0e-3, 1.0 - 1.0e-3)
//     opacity_loss = torch.nn.functional.binary_cross_entropy(opacity, opacity)
// as two launches forward and one backward over the RAW opacity x ([N], float32, or float64 from the first reset_opacity on):
//     o = sigmoid(x), c = min(max(o, lo), hi), inside = (lo <= o <= hi), lo / hi rounded to x's dtype like torch's clamp
//     value = mean h(c),   h(c) = -(c log c + (1 - c) log(1 - c))
//     dvalue/dx = (log(1 - c) - log c) * inside * o (1 - o) / N       (the cross entropy's input derivative is exactly 0)
// With e = exp(-|x|) both reduce to forms without a cancellation (neither 1 - o nor log o is formed from a rounded o):
//     inside:  h = log1p(e) + |x| e / (1 + e),   d = -x e / (1 + e)^2;     outside:  h = h(lo) or h(hi), d = 0
// and `inside` is lo <= sigmoid(x) <= hi decided on x itself: logit(lo) <= x <= logit(hi) (sigmoid is monotonic; which side
// an element within an ulp of a bound falls on differs between any two exp implementations anyway). NaN gives NaN in the
// value and in its own gradient element, +-Inf is outside.
// The arithmetic is float64 for BOTH input types, rounded once on the way out: the accuracy bar against the float64 formula
// is a few float32 ulps for a handful of elements, which a chain of float32 exp / log1p / divide does not keep. Measured
// cost: profiles/r8_opacity_entropy_ab.txt (the float32 kernels are VALU-bound rather than HBM-bound, and still a small
// fraction of the torch spelling they replace).
// opacity_entropy_fwd: grid-stride loop, 16-byte loads, one float64 partial per block with a plain store (no atomics);
// the grid depends on N alone. opacity_entropy_final: one workgroup sums the partials in a fixed order -> bit-reproducible.
// opacity_entropy_bwd reads x again (no N-sized scratch) and the upstream gradient from device memory.
#include "sfgs_internal.h"

#include <math.h>

namespace sfgs {

constexpr int OE_THREADS = 256;
constexpr int OE_MAX_BLOCKS = 2048;   // 8 workgroups on each of 256 CUs; also the most partials opacity_entropy_final sums

struct OeBounds {
  double x_lo, x_hi;   // logit(lo), logit(hi)
  double h_lo, h_hi;   // h(lo), h(hi)
};

template <typename T> struct OeVec;
template <> struct OeVec<float> { using type = float4; static constexpr int V = 4; };
template <> struct OeVec<double> { using type = double2; static constexpr int V = 2; };

template <typename T, int V>
__device__ __forceinline__ void oe_load(const T* __restrict__ p, long long i, double (&out)[V]) {
  if constexpr (V == 1) {
    out[0] = (double)p[i];
  } else {
    const typename OeVec<T>::type v = reinterpret_cast<const typename OeVec<T>::type*>(p)[i];
    if constexpr (V == 4) { out[0] = (double)v.x; out[1] = (double)v.y; out[2] = (double)v.z; out[3] = (double)v.w; }
    else { out[0] = (double)v.x; out[1] = (double)v.y; }
  }
}
template <typename T, int V>
__device__ __forceinline__ void oe_store(T* __restrict__ p, long long i, const double (&in)[V]) {
  if constexpr (V == 1) {
    p[i] = (T)in[0];
  } else if constexpr (V == 4) {
    reinterpret_cast<float4*>(p)[i] = make_float4((float)in[0], (float)in[1], (float)in[2], (float)in[3]);
  } else {
    reinterpret_cast<double2*>(p)[i] = make_double2(in[0], in[1]);
  }
}

__device__ __forceinline__ double oe_value(double x, const OeBounds& b) {
  if (x != x) return x;
  if (x < b.x_lo) return b.h_lo;
  if (x > b.x_hi) return b.h_hi;
  const double a = fabs(x), e = exp(-a);
  return log1p(e) + a * (e / (1.0 + e));
}
__device__ __forceinline__ double oe_deriv(double x, const OeBounds& b) {
  if (x != x) return x;
  if (x < b.x_lo || x > b.x_hi) return 0.0;
  const double e = exp(-fabs(x)), s = 1.0 + e;
  return -x * (e / (s * s));
}

template <typename T, int V>
__global__ void __launch_bounds__(OE_THREADS)
opacity_entropy_fwd_kernel(const T* __restrict__ x, long long n, OeBounds b, double* __restrict__ partials) {
  __shared__ double sm[OE_THREADS / 64];
  const long long nv = n / V, stride = (long long)gridDim.x * OE_THREADS;
  double acc = 0.0;
  for (long long i = (long long)blockIdx.x * OE_THREADS + threadIdx.x; i < nv; i += stride) {
    double v[V];
    oe_load<T, V>(x, i, v);
#pragma unroll
    for (int j = 0; j < V; ++j) acc += oe_value(v[j], b);
  }
  if (V > 1 && blockIdx.x == 0 && threadIdx.x < n - nv * V) acc += oe_value((double)x[nv * V + threadIdx.x], b);   // n % V
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_down(acc, d, 64);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < OE_THREADS / 64; ++w) t += sm[w];
    partials[blockIdx.x] = t;
  }
}

// ONE workgroup: strided per-thread sums, shuffle tree, the wave sums in wave order (the order of loss_final_kernel)
template <typename T>
__global__ void __launch_bounds__(1024)
opacity_entropy_final_kernel(const double* __restrict__ partials, int n_partials, double inv_n, T* __restrict__ out) {
  __shared__ double sm[16];
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int i = tid; i < n_partials; i += 1024) acc += partials[i];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_down(acc, d, 64);
  if ((tid & 63) == 0) sm[tid >> 6] = acc;
  __syncthreads();
  if (tid != 0) return;
  double t = 0.0;
  for (int w = 0; w < 16; ++w) t += sm[w];
  out[0] = (T)(t * inv_n);
}

template <typename T, int V>
__global__ void __launch_bounds__(OE_THREADS)
opacity_entropy_bwd_kernel(const T* __restrict__ x, long long n, OeBounds b, const T* __restrict__ grad_out, double inv_n,
                           T* __restrict__ grad) {
  const double scale = (double)grad_out[0] * inv_n;
  const long long nv = n / V, stride = (long long)gridDim.x * OE_THREADS;
  for (long long i = (long long)blockIdx.x * OE_THREADS + threadIdx.x; i < nv; i += stride) {
    double v[V];
    oe_load<T, V>(x, i, v);
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = scale * oe_deriv(v[j], b);
    oe_store<T, V>(grad, i, v);
  }
  if (V > 1 && blockIdx.x == 0 && threadIdx.x < n - nv * V) {
    const long long i = nv * V + threadIdx.x;
    grad[i] = (T)(scale * oe_deriv((double)x[i], b));
  }
}

}  // namespace sfgs

using namespace sfgs;

namespace {

struct OePlan {
  long long n;
  bool f64;
  int blocks;      // of both streaming kernels = partials of the forward: a function of n (and the dtype's vector) alone
  OeBounds b;
  size_t total;
};

inline double entropy(double c) { return -(c * log(c) + (1.0 - c) * log1p(-c)); }

int oe_plan(const SfgsOpacityEntropyArgs* a, OePlan* p) {
  SFGS_REQUIRE(a, SFGS_E_ARG, "NULL SfgsOpacityEntropyArgs");
  SFGS_REQUIRE(a->struct_size == sizeof(SfgsOpacityEntropyArgs), SFGS_E_ARG,
               "SfgsOpacityEntropyArgs.struct_size %u, expected %zu", a->struct_size, sizeof(SfgsOpacityEntropyArgs));
  SFGS_REQUIRE(a->n > 0, SFGS_E_ARG, "SfgsOpacityEntropyArgs.n %lld", (long long)a->n);
  SFGS_REQUIRE(a->opacity_raw, SFGS_E_ARG, "SfgsOpacityEntropyArgs.opacity_raw is NULL");
  p->n = a->n;
  p->f64 = a->is_f64 != 0;
  // torch's clamp takes its Python scalars in the tensor's dtype
  const double lo = p->f64 ? a->lo : (double)(float)a->lo, hi = p->f64 ? a->hi : (double)(float)a->hi;
  SFGS_REQUIRE(lo > 0.0 && lo < hi && hi < 1.0, SFGS_E_ARG, "SfgsOpacityEntropyArgs: need 0 < lo < hi < 1, got %g, %g",
               a->lo, a->hi);
  p->b.x_lo = log(lo) - log1p(-lo);
  p->b.x_hi = log(hi) - log1p(-hi);
  p->b.h_lo = entropy(lo);
  p->b.h_hi = entropy(hi);
  const long long per = (long long)OE_THREADS * (p->f64 ? 2 : 4);
  const long long want = (a->n + per - 1) / per;
  p->blocks = (int)(want < OE_MAX_BLOCKS ? want : OE_MAX_BLOCKS);
  p->total = align_up((size_t)p->blocks * sizeof(double), 256);
  return SFGS_OK;
}

inline bool oe_aligned16(const void* q) { return ((uintptr_t)q & 15u) == 0; }

}  // namespace

extern "C" size_t sfgs_opacity_entropy_scratch_bytes(const SfgsOpacityEntropyArgs* args) {
  OePlan p;
  return oe_plan(args, &p) == SFGS_OK ? p.total : 0;
}

extern "C" int sfgs_opacity_entropy_forward(const SfgsOpacityEntropyArgs* args, void* out_scalar, void* scratch,
                                            size_t scratch_bytes, void* stream_) {
  OePlan p;
  if (const int rc = oe_plan(args, &p)) return rc;
  SFGS_REQUIRE(out_scalar && scratch, SFGS_E_ARG, "NULL argument");
  SFGS_REQUIRE(scratch_bytes >= p.total, SFGS_E_CAPACITY, "opacity-entropy scratch too small: %zu < %zu", scratch_bytes,
               p.total);
  hipStream_t stream = (hipStream_t)stream_;
  double* partials = (double*)scratch;
  const bool vec = oe_aligned16(args->opacity_raw) && p.n >= (p.f64 ? 2 : 4);
  const dim3 grid((unsigned)p.blocks), block(OE_THREADS);
  { ProfScope ps_(KID_OPACITY_ENTROPY_FWD, stream);
    if (p.f64) {
      const double* x = (const double*)args->opacity_raw;
      if (vec) hipLaunchKernelGGL((opacity_entropy_fwd_kernel<double, 2>), grid, block, 0, stream, x, p.n, p.b, partials);
      else hipLaunchKernelGGL((opacity_entropy_fwd_kernel<double, 1>), grid, block, 0, stream, x, p.n, p.b, partials);
    } else {
      const float* x = (const float*)args->opacity_raw;
      if (vec) hipLaunchKernelGGL((opacity_entropy_fwd_kernel<float, 4>), grid, block, 0, stream, x, p.n, p.b, partials);
      else hipLaunchKernelGGL((opacity_entropy_fwd_kernel<float, 1>), grid, block, 0, stream, x, p.n, p.b, partials);
    } }
  SFGS_POST_LAUNCH("opacity_entropy_fwd", stream, 0);
  const double inv_n = 1.0 / (double)p.n;
  { ProfScope ps_(KID_OPACITY_ENTROPY_FINAL, stream);
    if (p.f64)
      hipLaunchKernelGGL(opacity_entropy_final_kernel<double>, dim3(1), dim3(1024), 0, stream, partials, p.blocks, inv_n,
                         (double*)out_scalar);
    else
      hipLaunchKernelGGL(opacity_entropy_final_kernel<float>, dim3(1), dim3(1024), 0, stream, partials, p.blocks, inv_n,
                         (float*)out_scalar); }
  SFGS_POST_LAUNCH("opacity_entropy_final", stream, 0);
  return SFGS_OK;
}

extern "C" int sfgs_opacity_entropy_backward(const SfgsOpacityEntropyArgs* args, const void* grad_out_scalar, void* grad_raw,
                                             void* stream_) {
  OePlan p;
  if (const int rc = oe_plan(args, &p)) return rc;
  SFGS_REQUIRE(grad_out_scalar && grad_raw, SFGS_E_ARG, "NULL argument");
  SFGS_REQUIRE(args->with_grad, SFGS_E_ARG, "sfgs_opacity_entropy_backward needs SfgsOpacityEntropyArgs.with_grad");
  hipStream_t stream = (hipStream_t)stream_;
  const bool vec = oe_aligned16(args->opacity_raw) && oe_aligned16(grad_raw) && p.n >= (p.f64 ? 2 : 4);
  const dim3 grid((unsigned)p.blocks), block(OE_THREADS);
  const double inv_n = 1.0 / (double)p.n;
  { ProfScope ps_(KID_OPACITY_ENTROPY_BWD, stream);
    if (p.f64) {
      const double* x = (const double*)args->opacity_raw;
      const double* g = (const double*)grad_out_scalar;
      if (vec) hipLaunchKernelGGL((opacity_entropy_bwd_kernel<double, 2>), grid, block, 0, stream, x, p.n, p.b, g, inv_n, (double*)grad_raw);
      else hipLaunchKernelGGL((opacity_entropy_bwd_kernel<double, 1>), grid, block, 0, stream, x, p.n, p.b, g, inv_n, (double*)grad_raw);
    } else {
      const float* x = (const float*)args->opacity_raw;
      const float* g = (const float*)grad_out_scalar;
      if (vec) hipLaunchKernelGGL((opacity_entropy_bwd_kernel<float, 4>), grid, block, 0, stream, x, p.n, p.b, g, inv_n, (float*)grad_raw);
      else hipLaunchKernelGGL((opacity_entropy_bwd_kernel<float, 1>), grid, block, 0, stream, x, p.n, p.b, g, inv_n, (float*)grad_raw);
    } }
  SFGS_POST_LAUNCH("opacity_entropy_bwd", stream, 0);
  return SFGS_OK;
}
