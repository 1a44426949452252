// ssim_tile.h -- device helpers of the 32 x 22 SSIM tile shared by ssim.hip and loss.hip: the window's weights, the tile
// geometry, buffer-descriptor addressing, halo staging, the XCD-contiguous workgroup -> tile map and the register
// sliding window. Both files build the same fma chain per moment from these, so their SSIM values agree bit for bit.
#pragma once
#include "sfgs_internal.h"

namespace sfgs {

// The window: every translation unit keeps its own __constant__ copy under its own name (a __constant__ array has a host-side
// shadow symbol: one name in two files would clash at link time) and hands it to window_weights().
#define SSIM_WINDOW_VALUES                                                                                     \
  {1.028380124e-03f, 7.598758209e-03f, 3.600077331e-02f, 1.093606874e-01f, 2.130055279e-01f, 2.660117149e-01f, \
   2.130055279e-01f, 1.093606874e-01f, 3.600077331e-02f, 7.598758209e-03f, 1.028380124e-03f}
// tile of ST x STY = 32 x 22 outputs: the 42 x 32 staged halo gives the horizontal pass exactly 32 rows x 8 groups of
// 4 columns = 256 items, one per thread (a 32 x 32 tile has 336: a second round in which 176 threads idle at the barrier);
// the vertical pass is 32 columns x 8 groups of 3 rows (24 >= 22). 31.7 KB of LDS and <= 96 registers: five
// workgroups per CU (32 x 32: three).
// (entry k of the window == entry 10 - k bit for bit: window() reads entries 0..5 only)
constexpr int ST = 32, STY = 22, SHALO = 5, SIN = ST + 2 * SHALO, SINY = STY + 2 * SHALO;  // 42 x 32
constexpr int SPITCH = SIN + 2;                          // LDS row pitch of the staged inputs
constexpr int SQ = 4, SQV = 3;                           // outputs per thread: horizontal pass, vertical pass
static_assert(SINY * (ST / SQ) == 256 && ST * ((STY + SQV - 1) / SQV) == 256, "one item per thread in both passes");
constexpr float SSIM_C1 = 0.01f * 0.01f, SSIM_C2 = 0.03f * 0.03f;

__device__ __forceinline__ float block_sum_256(float v, float* smem) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) smem[tid >> 6] = v;
  __syncthreads();
  return smem[0] + smem[1] + smem[2] + smem[3];
}

constexpr int SROUNDS = SINY / 4;   // staging rounds: wave w of the 4 stages halo row 4 r + w in round r, lane = column
static_assert(SINY % 4 == 0 && SIN <= 64 && SPITCH >= SIN, "a halo row is one wave's (partial) load");

// Global memory goes through buffer descriptors, one per image plane (wave-uniform): an access is descriptor + scalar
// byte offset (the row, or the tile origin) + ONE per-thread byte offset that every access of the thread shares, so
// the address arithmetic costs no VALU instruction -- flat addressing spent a 64-bit add per load and store, and these
// kernels are VALU-bound (profiles/r5_ssim_*.txt). A plane is at most 2^32 - 1 bytes (checked at the entry points).
using rsrc_t = __amdgpu_buffer_rsrc_t;
__device__ __forceinline__ rsrc_t plane_rsrc(const float* plane, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(plane), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ float bload(rsrc_t r, uint32_t voff, uint32_t soff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
__device__ __forceinline__ void bstore(float v, rsrc_t r, uint32_t voff, uint32_t soff) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v), r, voff, soff, 0);
}

// Staging: wave w of the 4 stages halo row 4 r + w in round r, lane = column. Rows are wave-uniform, so a row's byte
// offset and validity are scalars; the column offset (clamped into the row: always a valid address) is the thread's
// one vector offset. Two v_cndmask per element apply the zero padding on the way to LDS -- instead of an integer
// division, four compares and a 64-bit address per element.
struct HaloLane { uint32_t xoff; bool xin; };
__device__ __forceinline__ HaloLane halo_lane(int lane, int x0, int W) {
  const int gx = x0 - SHALO + lane;
  return {(uint32_t)min(max(gx, 0), W - 1) * 4u, lane < SIN && gx >= 0 && gx < W};
}
// byte offset of image row (clamped) `y0 - SHALO + row` within its plane, and whether that row exists
__device__ __forceinline__ uint32_t halo_row(int row, int y0, int H, int W, bool& yin) {
  const int gy = y0 - SHALO + row;
  yin = gy >= 0 && gy < H;
  return (uint32_t)min(max(gy, 0), H - 1) * (uint32_t)W * 4u;
}

// Workgroup -> tile. The hardware deals workgroups to the 8 XCDs round-robin by linear id, and each XCD has its own L2:
// with tile = workgroup id, the four neighbours whose halos overlap a tile's (10 of its 32 staged rows, 10 of its 42
// columns) run on OTHER XCDs and every XCD pulls its own copy of the shared lines through the fabric -- 2.7x the
// algorithmic bytes for the backward kernel. So XCD k takes the k-th CONTIGUOUS eighth of the tiles (row-major within a
// plane), in order: what it has in flight at any time is a band of a few tile rows, whose halos meet in its L2.
// Returns the tile's index in plane-major, row-major order (also the index of its partial sum).
struct SsimTile { int index, plane, x0, y0; };
__device__ __forceinline__ SsimTile ssim_tile(int tiles_x, int tiles_y) {
  const int L = (int)xcd_remap(blockIdx.x, gridDim.x);
  const int per_plane = tiles_x * tiles_y;
  const int plane = L / per_plane, rem = L - plane * per_plane;
  const int by = rem / tiles_x, bx = rem - by * tiles_x;
  return {L, plane, bx * ST, by * STY};
}

// hz row of tap k of the vertical window that starts at row ly0 <= STY - 1: only the taps of the output rows that do not
// exist (22, 23) can pass the last staged row, and only those pay for the clamp
__device__ __forceinline__ int vrow(int ly0, int k) {
  return k <= SINY - STY ? ly0 + k : min(ly0 + k, SINY - 1);
}

// out[q] = sum_k W[k] * v[q + k], k ascending (the order of a direct 11-tap sum)
// The window's six distinct weights (it is symmetric) in VECTOR registers: v_fmac_f32 with a scalar-register
// weight measures 9-15 % slower over the whole forward kernel than with a vector-register one
// (profiles/r5_ssim_steps.txt), and the compiler keeps a __constant__ table in scalar registers unless told otherwise.
struct WindowWeights { float w[6]; };
__device__ __forceinline__ WindowWeights window_weights(const float (&table)[11]) {
  WindowWeights r;
#pragma unroll
  for (int k = 0; k < 6; ++k) asm volatile("v_mov_b32 %0, %1" : "=v"(r.w[k]) : "s"(table[k]));
  return r;
}
template <int Q>
__device__ __forceinline__ void window(const WindowWeights& ww, const float (&v)[Q + 10], float (&out)[Q]) {
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    float a = 0.f;
#pragma unroll
    for (int k = 0; k < 11; ++k) a = fmaf(ww.w[k < 6 ? k : 10 - k], v[q + k], a);
    out[q] = a;
  }
}

}  // namespace sfgs
