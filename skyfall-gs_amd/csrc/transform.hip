// transform.hip -- sfgs_similarity_transform (include/sfgs.h spells the float32 sequence): x' = s R x + t applied to a trained
// Gaussian scene -- positions, scales (log space or activated), quaternions, the SH coefficients beyond DC (bands 1-3 by the
// real-SH rotation matrices D_1, D_2, D_3 in eval_sh's basis) and filter_3D. The reference has no counterpart: it trains every
// scene in a frame of its own (scene/dataset_readers.py:378-390) and never merges two.
// ONE kernel, one workgroup of TF_BLOCK threads per TF_BLOCK consecutive Gaussians. Rows of sh_rest are 12, 32 or 60 bytes
// per channel (up to 180 per Gaussian) and rows of xyz 12 bytes: a lane walking its own row in global memory would touch a
// wave's 11.5 KB with 45 strided dword accesses. Instead the workgroup's rows -- one contiguous stretch of global memory --
// go through LDS: 16-byte global loads, consecutive lanes on consecutive addresses, ds_write_b128; then lane i works on row i
// in LDS at a dword stride of 3 (K - 1) or 3 and writes its results over its own row; the stretch leaves the same way. 45, 9
// and 3 are odd: the 64 lanes of a ds_read_b32 / ds_write_b32 fall on 64 different banks. The 24 of degree 2 is not, and that
// degree pays an 8-way conflict on the LDS side (not measured: degree 3 is what the reference trains).
// LDS: 256 x (45 + 3) x 4 = 48 KiB at degree 3, three workgroups per CU (160 KiB); 128 rows (six per CU) measured 4-7 % slower,
// 512 (one per CU) 18-20 % (profiles/r15_transform_ab.txt). scaling and filter_3D are elementwise on the flat arrays; a
// quaternion is one 16-byte access per lane. The constants arrive by value in the kernel arguments (scalar loads). No
// atomics, no scratch; in place (out == in) is safe: a workgroup reads its whole stretch before the barrier and writes it
// after, and no two workgroups share a row. No profiler id (as the depthvis and metrics kernels).
#include "sfgs_internal.h"

namespace sfgs {

#ifndef SFGS_TF_BLOCK   // -DSFGS_TF_BLOCK=128 / 512: the block-size comparison of profiles/r15_transform_ab.txt
#define SFGS_TF_BLOCK 256
#endif
constexpr int TF_BLOCK = SFGS_TF_BLOCK;

// 16 bytes at 4-byte alignment: a view into a larger table need not start on a 16-byte boundary
typedef float tf_v4 __attribute__((ext_vector_type(4), aligned(4)));

// `count` floats from global memory into LDS (FULL: count == FULL_COUNT, known at compile time) and back
template <int FULL_COUNT>
__device__ __forceinline__ void tf_stage_in(const float* __restrict__ g, float* __restrict__ l, bool full, int count) {
  if (full) {
    constexpr int NV = FULL_COUNT / 4;
    static_assert(FULL_COUNT % 4 == 0, "a full block is a whole number of 16-byte pieces");
#pragma unroll
    for (int j = 0; j < (NV + TF_BLOCK - 1) / TF_BLOCK; ++j) {
      const int i = j * TF_BLOCK + (int)threadIdx.x;
      if (i < NV) {
        const tf_v4 v = reinterpret_cast<const tf_v4*>(g)[i];
        reinterpret_cast<float4*>(l)[i] = make_float4(v.x, v.y, v.z, v.w);
      }
    }
  } else {
    for (int i = threadIdx.x; i < count; i += TF_BLOCK) l[i] = g[i];
  }
}
template <int FULL_COUNT>
__device__ __forceinline__ void tf_stage_out(float* __restrict__ g, const float* __restrict__ l, bool full, int count) {
  if (full) {
    constexpr int NV = FULL_COUNT / 4;
#pragma unroll
    for (int j = 0; j < (NV + TF_BLOCK - 1) / TF_BLOCK; ++j) {
      const int i = j * TF_BLOCK + (int)threadIdx.x;
      if (i < NV) {
        const float4 v = reinterpret_cast<const float4*>(l)[i];
        tf_v4 o; o.x = v.x; o.y = v.y; o.z = v.z; o.w = v.w;
        reinterpret_cast<tf_v4*>(g)[i] = o;
      }
    }
  } else {
    for (int i = threadIdx.x; i < count; i += TF_BLOCK) g[i] = l[i];
  }
}

// out_i = sum_j D[i][j] in_j over one band of M = 2 l + 1 coefficients at row[first + j] (nk3: stride 3), sums in index order
template <int M, int STRIDE>
__device__ __forceinline__ void tf_band(float* __restrict__ row, const float* __restrict__ D) {
  float v[M], o[M];
#pragma unroll
  for (int j = 0; j < M; ++j) v[j] = row[j * STRIDE];
#pragma unroll
  for (int i = 0; i < M; ++i) {
    float acc = D[i * M] * v[0];
#pragma unroll
    for (int j = 1; j < M; ++j) acc = acc + D[i * M + j] * v[j];
    o[i] = acc;
  }
#pragma unroll
  for (int i = 0; i < M; ++i) row[i * STRIDE] = o[i];
}

template <int KR, bool N3K>
__global__ void __launch_bounds__(TF_BLOCK)
similarity_kernel(const SfgsSimilarityArgs a) {
  constexpr int ROW = 3 * KR;
  __shared__ __attribute__((aligned(16))) float sh_lds[KR ? TF_BLOCK * ROW : 4];
  __shared__ __attribute__((aligned(16))) float xyz_lds[TF_BLOCK * 3];
  const long long g0 = (long long)blockIdx.x * TF_BLOCK;
  const long long left = a.n - g0;
  const int nb = left < TF_BLOCK ? (int)left : TF_BLOCK;   // >= 1: the grid is ceil(n / TF_BLOCK)
  const bool full = nb == TF_BLOCK;
  const int tid = threadIdx.x;
  const bool do_sh = KR > 0 && a.sh_rest_in != nullptr;
  const bool do_xyz = a.xyz_in != nullptr;
  if (do_sh) tf_stage_in<TF_BLOCK * (KR ? ROW : 4)>(a.sh_rest_in + (size_t)g0 * ROW, sh_lds, full, nb * ROW);
  if (do_xyz) tf_stage_in<TF_BLOCK * 3>(a.xyz_in + (size_t)g0 * 3, xyz_lds, full, nb * 3);
  // elementwise tensors: this workgroup's stretch of the flat arrays
  if (a.scaling_in) {
    const float* in = a.scaling_in + (size_t)g0 * 3;
    float* out = a.scaling_out + (size_t)g0 * 3;
    const bool is_log = (a.flags & SFGS_SIM_SCALING_LOG) != 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int i = j * TF_BLOCK + tid;
      if (i < nb * 3) {
        const float v = in[i];
        out[i] = is_log ? v + a.log_s : v * a.s;
      }
    }
  }
  if (tid < nb) {
    const size_t g = (size_t)g0 + tid;
    if (a.filter3d_in) a.filter3d_out[g] = a.filter3d_in[g] * a.s;
    if (a.rotation_in) {
      const tf_v4 b = reinterpret_cast<const tf_v4*>(a.rotation_in)[g];   // (w, x, y, z)
      const float aw = a.q[0], ax = a.q[1], ay = a.q[2], az = a.q[3];
      tf_v4 o;
      o.x = ((aw * b.x - ax * b.y) - ay * b.z) - az * b.w;
      o.y = ((aw * b.y + ax * b.x) + ay * b.w) - az * b.z;
      o.z = ((aw * b.z - ax * b.w) + ay * b.x) + az * b.y;
      o.w = ((aw * b.w + ax * b.z) - ay * b.y) + az * b.x;
      reinterpret_cast<tf_v4*>(a.rotation_out)[g] = o;
    }
  }
  if (!do_sh && !do_xyz) return;   // uniform: no barrier is skipped by part of the workgroup
  __syncthreads();
  if (tid < nb) {
    if (do_xyz) {
      float* p = xyz_lds + tid * 3;
      const float x = p[0], y = p[1], z = p[2];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const float r = (a.R[3 * i] * x + a.R[3 * i + 1] * y) + a.R[3 * i + 2] * z;
        p[i] = a.s * r + a.t[i];
      }
    }
    if (do_sh) {
      float* row = sh_lds + tid * (KR ? ROW : 1);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float* ch = N3K ? row + c * KR : row + c;      // coefficient k of channel c: ch[k * STRIDE]
        constexpr int STRIDE = N3K ? 1 : 3;
        if (KR >= 3) tf_band<3, STRIDE>(ch, a.D1);
        if (KR >= 8) tf_band<5, STRIDE>(ch + 3 * STRIDE, a.D2);
        if (KR >= 15) tf_band<7, STRIDE>(ch + 8 * STRIDE, a.D3);
      }
    }
  }
  __syncthreads();
  if (do_sh) tf_stage_out<TF_BLOCK * (KR ? ROW : 4)>(a.sh_rest_out + (size_t)g0 * ROW, sh_lds, full, nb * ROW);
  if (do_xyz) tf_stage_out<TF_BLOCK * 3>(a.xyz_out + (size_t)g0 * 3, xyz_lds, full, nb * 3);
}

}  // namespace sfgs

using namespace sfgs;

namespace {

template <int KR>
void tf_launch(bool n3k, unsigned blocks, hipStream_t stream, const SfgsSimilarityArgs& a) {
  if (n3k) hipLaunchKernelGGL((similarity_kernel<KR, true>), dim3(blocks), dim3(TF_BLOCK), 0, stream, a);
  else hipLaunchKernelGGL((similarity_kernel<KR, false>), dim3(blocks), dim3(TF_BLOCK), 0, stream, a);
}

}  // namespace

extern "C" int sfgs_similarity_transform(const SfgsSimilarityArgs* args, void* stream_) {
  SFGS_REQUIRE(args, SFGS_E_ARG, "NULL SfgsSimilarityArgs");
  SFGS_REQUIRE(args->struct_size == sizeof(SfgsSimilarityArgs), SFGS_E_ARG, "SfgsSimilarityArgs.struct_size %u, expected %zu",
               args->struct_size, sizeof(SfgsSimilarityArgs));
  SFGS_REQUIRE(args->n >= 0, SFGS_E_ARG, "SfgsSimilarityArgs.n %lld", (long long)args->n);
  SFGS_REQUIRE(args->n < (1ll << 31), SFGS_E_UNSUPPORTED, "SfgsSimilarityArgs.n %lld: at most 2^31 - 1 Gaussians per call",
               (long long)args->n);
  SFGS_REQUIRE((args->flags & ~(SFGS_SIM_SCALING_LOG | SFGS_SIM_REST_N3K)) == 0, SFGS_E_ARG,
               "SfgsSimilarityArgs.flags %d has an unknown bit", args->flags);
  const int kr = args->sh_rest_coeffs;
  SFGS_REQUIRE(kr == 0 || kr == 3 || kr == 8 || kr == 15, SFGS_E_ARG,
               "SfgsSimilarityArgs.sh_rest_coeffs %d: 0, 3, 8 or 15 (SH degree 0 to 3)", kr);
  SFGS_REQUIRE(kr > 0 || !args->sh_rest_in, SFGS_E_ARG, "SfgsSimilarityArgs: sh_rest_in with sh_rest_coeffs 0");
  SFGS_REQUIRE((!args->xyz_in || args->xyz_out) && (!args->scaling_in || args->scaling_out) &&
               (!args->rotation_in || args->rotation_out) && (!args->sh_rest_in || args->sh_rest_out) &&
               (!args->filter3d_in || args->filter3d_out), SFGS_E_ARG, "SfgsSimilarityArgs: an input without its output");
  const bool any = args->xyz_in || args->scaling_in || args->rotation_in || args->sh_rest_in || args->filter3d_in;
  if (args->n == 0 || !any) return SFGS_OK;
  hipStream_t stream = (hipStream_t)stream_;
  const unsigned blocks = (unsigned)((args->n + TF_BLOCK - 1) / TF_BLOCK);
  const bool n3k = (args->flags & SFGS_SIM_REST_N3K) != 0;
  switch (args->sh_rest_in ? kr : 0) {   // without the table the kernel needs none of its LDS
    case 3: tf_launch<3>(n3k, blocks, stream, *args); break;
    case 8: tf_launch<8>(n3k, blocks, stream, *args); break;
    case 15: tf_launch<15>(n3k, blocks, stream, *args); break;
    default: tf_launch<0>(false, blocks, stream, *args); break;
  }
  SFGS_POST_LAUNCH("similarity", stream, 0);
  return SFGS_OK;
}
