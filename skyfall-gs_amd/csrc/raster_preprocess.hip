// raster_preprocess.hip -- first stage of the forward's plan (map of the forward: raster_fwd.hip): subpix_bound ->
// preprocess (per Gaussian: project, radii, 48-B record; opacity-aware COARSE binning: one 16-B item per (Gaussian,
// 32x32-px coarse bin) with the mask of the 8x8 tiles it can contribute to) -> big_walk (the splats of 64 coarse bins
// and more, one wave per splat). preprocess_kernel is instantiated over every SH layout: most of the forward's compile
// time is this file.
//
// Compile with -ffp-contract=off: integer outputs depend on exact float32 sequences (raster_math.h).
#include <algorithm>

#include "act_math.h"
#include "sfgs_internal.h"

namespace sfgs {

// Variant built, measured and not kept (A/B file; the code is in the history, not in this source):
//   preprocess: records leave through LDS as lane-contiguous stores         profiles/r4_preprocess_rec_transpose_ab_not_kept.txt

// ------------------------------------------------------------------------------------------------
// max |subpixel_offset| -> header (float bits; non-negative floats order like unsigned ints)
__global__ void __launch_bounds__(256) subpix_bound_kernel(const float* __restrict__ subpix, int64_t n,
                                                           unsigned long long* __restrict__ hdr) {
  // float4 loads, a few hundred workgroups, ONE atomic per workgroup and none at all for an all-zero tensor (what the
  // reference's render() passes when ray jitter is off): atomics to one address serialise at ~12 ns each
  __shared__ float s_m[4];
  float m = 0.f;
  const int64_t n4 = (reinterpret_cast<uintptr_t>(subpix) & 15) ? 0 : (n >> 2);  // unaligned view: scalar tail only
  const float4* __restrict__ v4 = reinterpret_cast<const float4*>(subpix);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 v = v4[i];
    m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
  }
  for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    m = fmaxf(m, fabsf(subpix[i]));
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
  if (lane_id() == 0) s_m[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3]));
    if (m > 0.f) atomicMax((unsigned int*)&hdr[HDR_SUBPIX_BOUND], __float_as_uint(m));
  }
}

// 16-bit hit mask of the 4x4 tiles of coarse bin (cbx, cby) that lie inside the walk range `br`
// (bit = 4 * local_y + local_x).
__device__ __forceinline__ unsigned coarse_hits(const SplatRec& r, float thr, const BinRange& br, int cbx, int cby,
                                                int W, int H, float bound) {
  unsigned m = 0;
  const int tx0 = imax(br.x0, cbx * COARSE), tx1 = imin(br.x1, cbx * COARSE + COARSE);
  const int ty0 = imax(br.y0, cby * COARSE), ty1 = imin(br.y1, cby * COARSE + COARSE);
  for (int ty = ty0; ty < ty1; ++ty)
    for (int tx = tx0; tx < tx1; ++tx)
      if (bin_test(r, thr, tx, ty, W, H, bound)) m |= 1u << ((ty - cby * COARSE) * COARSE + (tx - cbx * COARSE));
  return m;
}

// small walks handed to the wave (preprocess_kernel): at most this many tiles per Gaussian (so a wave has at most 2 048
// tasks), the owner's test inputs, its mask words and the task -> owner map, 7 KB of LDS per wave
constexpr int WALK_COOP_MAX = 32;
struct WalkLds {
  float4 rec[64][4];
  uint4 mask[64];
  unsigned char owner[64 * WALK_COOP_MAX];
};
constexpr int BIG_WALK = 6;  // coarse bins above which a splat's walk is done by a whole wave (big_walk_kernel)
constexpr int BIG_WALK_BLOCKS = 1024;   // persistent grid of big_walk_kernel: 4 096 waves = 4 per SIMD, what its 120 VGPRs allow (round 4:
                                        // with 1 per SIMD nothing hid the tile tests' dependent chains -- near-camera regime); the
                                        // kernel is not launched at all under the NO_HUGE_SPLATS hint
constexpr int BIG_WALK_CACHE = 2048;    // coarse-bin masks a wave keeps in LDS between its count and emit passes (16-bit each)
static_assert(BIG_WALK <= 8, "the per-lane walk keeps one 16-bit mask per coarse bin in two 64-bit registers");

struct WalkArgs { SplatRec r; BinRange br; float thr; int cx0, cx1, cy0, cy1; };

// lane L's walk parameters, broadcast to the wave
__device__ __forceinline__ WalkArgs broadcast_walk(const SplatRec& r, const BinRange& br, float thr, int cx0, int cx1,
                                                  int cy0, int cy1, int L) {
  WalkArgs a;
  a.r.mx = __shfl(r.mx, L); a.r.my = __shfl(r.my, L); a.r.qa = __shfl(r.qa, L); a.r.qb = __shfl(r.qb, L);
  a.r.qc = __shfl(r.qc, L); a.r.op = __shfl(r.op, L); a.r.depth = 0.f; a.r.r = a.r.g = a.r.b = 0.f;
  a.r.ex = __shfl(r.ex, L); a.r.ey = __shfl(r.ey, L);
  a.br.x0 = __shfl(br.x0, L); a.br.x1 = __shfl(br.x1, L); a.br.y0 = __shfl(br.y0, L); a.br.y1 = __shfl(br.y1, L);
  a.thr = __shfl(thr, L);
  a.cx0 = __shfl(cx0, L); a.cx1 = __shfl(cx1, L); a.cy0 = __shfl(cy0, L); a.cy1 = __shfl(cy1, L);
  return a;
}

// Cooperative walk, lane = TILE: lanes 16q..16q+15 test the 16 tiles of coarse bin number 4*it + q of the walk
// (row-major over [cx0,cx1) x [cy0,cy1)); the ballot's 16-bit slice q is that bin's mask, identical to coarse_hits().
// A mid-size splat (6..63 coarse bins) keeps all 64 lanes busy this way; one lane per coarse bin would use 6..63.
__device__ __forceinline__ unsigned long long walk_ballot4(const WalkArgs& a, int it, int lane, int W, int H,
                                                           float bound, int* cb_index, int CX) {
  const int nx = a.cx1 - a.cx0, ncb = nx * (a.cy1 - a.cy0);
  const int i = it * 4 + (lane >> 4), t = lane & 15;
  bool hit = false;
  int cb = 0;
  if (i < ncb) {
    const int cx = a.cx0 + i % nx, cy = a.cy0 + i / nx;
    const int tx = cx * COARSE + (t & (COARSE - 1)), ty = cy * COARSE + (t / COARSE);
    cb = cy * CX + cx;
    if (tx >= a.br.x0 && tx < a.br.x1 && ty >= a.br.y0 && ty < a.br.y1) hit = bin_test(a.r, a.thr, tx, ty, W, H, bound);
  }
  *cb_index = cb;
  return __ballot(hit);
}

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += (unsigned)__shfl_xor((int)v, d);
  return v;
}

// ------------------------------------------------------------------------------------------------
// K1: one thread per Gaussian: project, write radii + the compositing record, and bin COARSELY.
// The thread walks the coarse bins (32x32 px) its splat can reach; for each it computes the 16-bit mask of
// the 8x8 tiles the splat can contribute to (opacity-aware test, raster_math.h). A non-empty mask becomes
// one 16-byte coarse item (id, depth, first duplicate index, mask) appended to the bin's slab with ONE
// returning device atomic. The block reserves its duplicate indices (one per set mask bit, in walk order)
// with one atomic per block.
// RAW: `scales`, `rots`, `opac` are the model's raw parameters and `filt` its 3D filter (SfgsGaussians raw-parameter
// mode): the activations of act_math.h run here instead of in a pre-pass kernel that writes N-sized intermediates.
// CM != 0 (SfgsGaussians.sh_dirs): the view direction of a Gaussian is read from `sh_dirs` -- the eval_sh + 0.5 +
// clamp_min of render()'s Python colour paths folded in (sh_to_rgb); CM == 1: `shs` is channel-major [N,3,K] (eval_sh's
// layout), CM == 2: coefficient-major [N,K,3].
template <int K, int DEG, bool RAW, int CM>  // K = SH coefficients stored per Gaussian (0: colors_precomp), DEG = active degree
__global__ void __launch_bounds__(PRE_BLOCK)
preprocess_kernel(KFrame kf, int N, const float* __restrict__ means3D, const float* __restrict__ scales,
                  const float* __restrict__ rots, const void* __restrict__ opac_, const void* __restrict__ filt,
                  int raw_mask,
                  const float* __restrict__ colors, const float* __restrict__ shs, const float* __restrict__ shs_rest,
                  const float* __restrict__ sh_dirs, int dirs_are_centers, int* __restrict__ radii,
                  float4* __restrict__ rec_out, uint2* __restrict__ dup_out, uint32_t* __restrict__ coarse_count,
                  uint4* __restrict__ slabs, unsigned coarse_capacity, unsigned long long dup_capacity,
                  uint32_t* __restrict__ block_nvis, unsigned long long* __restrict__ block_dref,
                  uint4* __restrict__ big_list, unsigned long long* __restrict__ hdr,
                  unsigned long long* __restrict__ dup_pool, uint4* __restrict__ pairs,
                  uint32_t* __restrict__ block_items) {
  __shared__ unsigned s_red[PRE_BLOCK / 64 + 1];
  __shared__ unsigned long long s_base;
  const FrameParams f = load_frame(kf);
  const float bound = __uint_as_float((unsigned)hdr[HDR_SUBPIX_BOUND]);
  const int g = blockIdx.x * PRE_BLOCK + threadIdx.x;
  const int CX = (((f.W + TILE_BIN - 1) / TILE_BIN) + COARSE - 1) / COARSE;
  unsigned n_dup = 0, vis = 0, dref = 0, depth_bits = 0;
  unsigned long long mask_lo = 0ull, mask_hi = 0ull;  // 16-bit tile masks of the (<= BIG_WALK) coarse bins of the walk
  unsigned walk_tiles = 0;           // tiles of a walk of at most BIG_WALK coarse bins (<= 96): walked after the per-thread part
  bool big = false;                  // walk handled cooperatively by the wave (BIG_WALK < coarse bins < 64)
  bool huge = false;                 // >= 64 coarse bins: walked by big_walk_kernel
  const int lane = threadIdx.x & 63;
  SplatRec r;
  BinRange br;
  float thr = 0.f;
  int cx0 = 0, cx1 = 0, cy0 = 0, cy1 = 0;
  br.x0 = br.x1 = br.y0 = br.y1 = 0;
  if (g < N) {
    // every input of the Gaussian is requested before the first one is used (the empty asm below consumes one word of
    // each load, which keeps the compiler from sinking the loads behind the near-plane test inside project_gaussian and
    // behind `if (pr.visible)`: three dependent round trips to memory per thread otherwise)
    float p[3], s[3];
    load3(means3D + 3 * (size_t)g, p);
    load3(scales + 3 * (size_t)g, s);
    float4 qv = *reinterpret_cast<const float4*>(rots + 4 * (size_t)g);
    float opacity_in = 0.f;
    if constexpr (!RAW) opacity_in = static_cast<const float*>(opac_)[g];
    float rgb_in[3] = {0.f, 0.f, 0.f};
    if constexpr (K == 0) load3(colors + 3 * (size_t)g, rgb_in);
    // RAW: the raw opacity and filter_3D words belong to the same round trip (as bits: their types are a launch-uniform
    // switch, and a load inside the switch BELOW the asm would be a second, dependent trip to memory)
    unsigned long long o_bits = 0ull, f_bits = 0ull;
    if constexpr (RAW) {
#define SFGS_ACT_LOAD(FT, OT) do { o_bits = raw_bits<OT>(opac_, g); f_bits = raw_bits<FT>(filt, g); } while (0)
      SFGS_ACT_DISPATCH(raw_mask, SFGS_ACT_LOAD);
#undef SFGS_ACT_LOAD
    }
    asm volatile("" :: "v"(p[2]), "v"(s[0]), "v"(qv.x), "v"(opacity_in), "v"(rgb_in[0]), "v"((unsigned)o_bits),
                 "v"((unsigned)f_bits));   // all of them in registers here
    if constexpr (RAW) {   // raw parameters -> what render() would have passed (the mask is uniform over the launch)
#define SFGS_ACT_FWD(FT, OT) act_outputs(act_terms<FT, OT>(s, from_bits<OT>(o_bits), from_bits<FT>(f_bits)), s, &opacity_in)
      SFGS_ACT_DISPATCH(raw_mask, SFGS_ACT_FWD);
#undef SFGS_ACT_FWD
      qv = act_rotation(qv);
    }
    float q[4] = {qv.x, qv.y, qv.z, qv.w};
    const Projected pr = project_gaussian(f, p, s, q);
    radii[g] = pr.radius;
    if (pr.visible) {
      vis = 1;
      dref = (unsigned)((pr.rmaxx - pr.rminx) * (pr.rmaxy - pr.rminy));
      float rgb[3];
      if constexpr (K == 0) {
        rgb[0] = rgb_in[0]; rgb[1] = rgb_in[1]; rgb[2] = rgb_in[2];
      } else {
        float shl[3 * K];
        // coefficient-major rows: K 12-byte loads from one array or, split storage (SfgsGaussians.shs_rest), from two --
        // the same instructions either way (load_sh_rows); the channel-major form [N,3,K] reads its 3 K floats as they lie
        if constexpr (K > 1 && CM != 1) load_sh_rows<K>(shs, shs_rest, (size_t)g, shl);
        else load_row<3 * K>(shs + 3 * (size_t)K * g, shl);
        unsigned cm; float dir[3], len;
        if constexpr (CM != 0) {
          float din[3];
          load3(sh_dirs + 3 * (size_t)g, din);
          // dirs_are_centers (SfgsGaussians.sh_centers): `sh_dirs` holds per-Gaussian centres c and the direction is
          // normalize(p - c), computed here like the in-kernel SH path's normalize(p - campos); wave-uniform
          sh_to_rgb(DEG, shl, p, dirs_are_centers ? din : f.campos, rgb, &cm, dir, &len, CM == 1 ? 1 : 3, CM == 1 ? K : 1,
                    dirs_are_centers ? nullptr : din);
        } else {
          sh_to_rgb(DEG, shl, p, f.campos, rgb, &cm, dir, &len);
        }
      }
      r = make_record(pr, opacity_in, rgb);
      rec_out[REC_F4 * (size_t)g + 0] = make_float4(r.mx, r.my, r.qa, r.qb);
      // (r, g) and (b, depth) sit in aligned pairs: the compositing loops fetch them with one 16-byte and one 8-byte
      // LDS read into the register pairs their packed multiply-adds take
      rec_out[REC_F4 * (size_t)g + 1] = make_float4(r.qc, r.op, r.r, r.g);
      rec_out[REC_F4 * (size_t)g + 2] = make_float4(r.b, r.depth, r.ex, r.ey);
      depth_bits = __float_as_uint(r.depth);
      br = bin_range(r, f.W, f.H, pr.rminx, pr.rminy, pr.rmaxx, pr.rmaxy, bound);
      br.y0 = imax(br.y0, kf.band0); br.y1 = imax(br.y0, imin(br.y1, kf.band1));  // band rendering
      thr = alpha_threshold_log2(r.op);
      if (br.x1 > br.x0 && br.y1 > br.y0) {
        cx0 = br.x0 / COARSE; cx1 = (br.x1 - 1) / COARSE + 1;
        cy0 = br.y0 / COARSE; cy1 = (br.y1 - 1) / COARSE + 1;
        const int ncb_ = (cx1 - cx0) * (cy1 - cy0);
        huge = ncb_ >= 64;
        big = ncb_ > BIG_WALK && !huge;
        if (ncb_ <= BIG_WALK) {
          walk_tiles = (unsigned)(br.y1 - br.y0) * (unsigned)(br.x1 - br.x0);   // walked below, by the wave or by this thread
        }
      }
    }
  }
  // Small walks, balanced over the wave. One thread walking ITS Gaussian's tiles makes the wave run max over its 64
  // lanes of the tile counts -- 11.4 steps on the headline scene for 4.4 tiles per Gaussian (tools/workmodel) -- in a kernel
  // that is bound by VALU issue with this loop as half of its instructions. Here lane = one (Gaussian, tile) task: the
  // owners publish what the test needs (48 bytes) and their lane number in the task slots they own, every lane takes task
  // 64 p + lane in pass p (4.9 passes), hits are ORed into the owner's mask words with LDS atomics. Same tests on the
  // same tiles: masks and duplicate counts are bit-identical.
  // A walk of more than WALK_COOP_MAX tiles (33 .. 96: its tasks would not fit the wave's task map) is not left to its
  // owner thread -- until round 6 such a lane sent its WHOLE wave back to the thread-per-Gaussian loop, up to 96 serial tile
  // tests with 63 lanes waiting: most waves of a low-elevation or UHD frame (preprocess 0.078 -> 0.276 ms on the pitched
  // camera) -- but walked by the whole wave, lane = tile, as the mid-size splats below are: its at most 6 coarse bins are
  // two ballots, whose 16-bit slices ARE the owner's mask words (walk_ballot4: same tests, same bit positions).
  const bool wide = walk_tiles > (unsigned)WALK_COOP_MAX;
  const unsigned long long wide_lanes = __ballot(wide);
  if (wide) walk_tiles = 0;   // not a task of the cooperative map
  for (unsigned long long wl_ = wide_lanes; wl_; wl_ &= wl_ - 1) {
    const int L = __builtin_ctzll(wl_);
    const WalkArgs a = broadcast_walk(r, br, thr, cx0, cx1, cy0, cy1, L);
    int cb_;
    const unsigned long long m0 = walk_ballot4(a, 0, lane, f.W, f.H, bound, &cb_, CX);
    const unsigned long long m1 = (a.cx1 - a.cx0) * (a.cy1 - a.cy0) > 4 ? walk_ballot4(a, 1, lane, f.W, f.H, bound, &cb_, CX) : 0ull;
    if (lane == L) { mask_lo = m0; mask_hi = m1; n_dup = (unsigned)__popcll(m0) + (unsigned)__popcll(m1); }
  }
  {
    __shared__ WalkLds s_walk[PRE_BLOCK / 64];
    const unsigned incl = wave_incl_scan_u32(walk_tiles);
    const unsigned total_t = (unsigned)__builtin_amdgcn_readlane((int)incl, 63);
    if (total_t) {   // wave-uniform
      WalkLds& wl = s_walk[threadIdx.x >> 6];
      const unsigned excl = incl - walk_tiles;
      wl.mask[lane] = make_uint4(0u, 0u, 0u, 0u);
      if (walk_tiles) {
        const unsigned w_t = (unsigned)(br.x1 - br.x0);
        wl.rec[lane][0] = make_float4(r.mx, r.my, r.qa, r.qb);
        wl.rec[lane][1] = make_float4(r.qc, thr, (float)(br.x0 * TILE_BIN), (float)(br.y0 * TILE_BIN));
        // k / w_t for k < 32 as (k * M) >> 16 with M = ceil(2^16 / w_t): exact while k (M - 2^16 / w_t) < 2^16 / w_t
        const unsigned M = (65536u + w_t - 1u) / w_t;
        wl.rec[lane][2] = make_float4(__uint_as_float(w_t | (M << 8)), __uint_as_float((unsigned)br.x0 | ((unsigned)br.y0 << 16)),
                                      __uint_as_float((unsigned)cx0 | ((unsigned)cy0 << 16)),
                                      __uint_as_float((unsigned)(cx1 - cx0) | (excl << 8)));
        wl.rec[lane][3] = make_float4(-0.5f / r.qc, -0.5f / r.qa, 0.f, 0.f);   // the test's two divisions, once per Gaussian
        for (unsigned k = 0; k < walk_tiles; ++k) wl.owner[excl + k] = (unsigned char)lane;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const float wm1 = (float)(f.W - 1), hm1 = (float)(f.H - 1);
      for (unsigned t0 = 0; t0 < total_t; t0 += 64) {
        const unsigned t = t0 + (unsigned)lane;
        if (t < total_t) {
          const unsigned o = wl.owner[t];
          const float4 a0 = wl.rec[o][0], a1 = wl.rec[o][1], a2 = wl.rec[o][2];
          const float2 a3 = *reinterpret_cast<const float2*>(&wl.rec[o][3]);
          const unsigned wM = __float_as_uint(a2.x), xy = __float_as_uint(a2.y), cxy = __float_as_uint(a2.z),
                         ne = __float_as_uint(a2.w);
          const unsigned w_t = wM & 0xffu, k = t - (ne >> 8);
          const unsigned row = __umul24(k, wM >> 8) >> 16, col = k - __umul24(row, w_t);   // k < 32, M <= 2^16
          SplatRec q;
          q.mx = a0.x; q.my = a0.y; q.qa = a0.z; q.qb = a0.w; q.qc = a1.x;
          if (bin_test_at_h(q, a1.y, a1.z + (float)(col * TILE_BIN), a1.w + (float)(row * TILE_BIN), wm1, hm1, bound, a3.x, a3.y)) {
            const unsigned tx = (xy & 0xffffu) + col, ty = (xy >> 16) + row;
            const unsigned slot = ((ty >> 2) - (cxy >> 16)) * (ne & 0xffu) + ((tx >> 2) - (cxy & 0xffffu));
            const unsigned pos = slot * 16u + (ty & 3u) * 4u + (tx & 3u);
            atomicOr(&wl.mask[o].x + (pos >> 5), 1u << (pos & 31u));
          }
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (walk_tiles) {
        const uint4 m = wl.mask[lane];
        mask_lo = (unsigned long long)m.x | ((unsigned long long)m.y << 32);
        mask_hi = (unsigned long long)m.z;
        n_dup = (unsigned)__popcll(mask_lo) + (unsigned)__popc(m.z);
      }
      __builtin_amdgcn_wave_barrier();   // the next user of this wave's LDS block is the next launch
    }
  }
  // Mid-size splats (more than BIG_WALK, fewer than 64 coarse bins) are walked by the whole wave, lane = tile, instead
  // of serially by their owner thread.
  const unsigned long long big_lanes = __ballot(big);
  for (unsigned long long bl = big_lanes; bl; bl &= bl - 1) {
    const int L = __builtin_ctzll(bl);
    const WalkArgs a = broadcast_walk(r, br, thr, cx0, cx1, cy0, cy1, L);
    const int ncb = (a.cx1 - a.cx0) * (a.cy1 - a.cy0);
    unsigned total = 0;
    for (int it = 0; it * 4 < ncb; ++it) {
      int cb;
      total += (unsigned)__popcll(walk_ballot4(a, it, lane, f.W, f.H, bound, &cb, CX));
    }
    if (lane == L) n_dup = total;
  }
  // Huge splats (64 coarse bins and more, up to the whole screen) are not walked here: they go to the work list of
  // big_walk_kernel, which spreads them over the whole chip one wave per splat (walked by the wave that owns them,
  // 2 000 screen-filling splats kept 8 waves busy for 10 ms while the other 4 000 wave slots idled). That kernel also
  // reserves their duplicate indices and writes their dup_out entry.
  const unsigned long long huge_lanes = __ballot(huge);
  if (huge_lanes) {
    unsigned long long slot0 = 0ull;
    if (lane == 0) slot0 = atomicAdd(&hdr[HDR_BIG_COUNT], (unsigned long long)__popcll(huge_lanes));
    const unsigned s_lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)slot0);
    if (huge) {
      const unsigned rk = __builtin_amdgcn_mbcnt_hi((unsigned)(huge_lanes >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)huge_lanes, 0u));
      big_list[s_lo + rk] = make_uint4((unsigned)g, (unsigned)br.x0 | ((unsigned)br.x1 << 16),
                                       (unsigned)br.y0 | ((unsigned)br.y1 << 16), 0u);
    }
  }
  // reserve duplicate indices: block scan + one returning atomic per block. Two-pass binning (`pairs`): the same scan
  // ranks the thread's coarse ITEMS inside the workgroup's stretch of the pair list -- packed into one word: a
  // workgroup has < 2^20 duplicates (256 threads x at most 63 coarse bins x 16 tiles) and at most 1 536 own items
  unsigned n_items = 0;
  if (pairs && n_dup && !big && !huge) {
#pragma unroll
    for (int k = 0; k < BIG_WALK; ++k)
      n_items += ((k < 4 ? mask_lo >> (16 * k) : mask_hi >> (16 * (k - 4))) & 0xffffull) != 0ull;
  }
  static_assert(PAIRS_PER_BLOCK == PRE_BLOCK * BIG_WALK, "a thread emits at most BIG_WALK items itself");
  unsigned total;
  const unsigned ex_packed = block_excl_scan_u32<PRE_BLOCK>(n_dup | (n_items << 20), &total, s_red);
  const unsigned ex = ex_packed & 0xfffffu, ex_items = ex_packed >> 20, total_items = total >> 20;
  total &= 0xfffffu;
  __shared__ int s_fits;
  if (threadIdx.x == 0) {
    bool ok = true;
    s_base = total ? dup_alloc(dup_pool, dup_pools_used(gridDim.x), blockIdx.x, total, dup_capacity, &ok) : 0ull;
    s_fits = ok;
  }
  __syncthreads();
  const unsigned long long base = s_base;
  const bool fits = s_fits != 0;
  if (!fits && threadIdx.x == 0) hdr[HDR_OVERFLOW] = 1ull;
  if (g < N && !huge) dup_out[g] = make_uint2((unsigned)(base + ex), n_dup);
  {
    // Emission, one coarse bin of the walk per iteration and lane. Lanes that append to the SAME bin in the same
    // iteration -- the rule rather than the exception when the Gaussians are stored in a spatially coherent order
    // (a loaded point cloud, clones next to their parents): 64 returning atomics on one counter serialise, the kernel
    // was 2.5x slower on a Z-curve-ordered scene than on a shuffled one -- are merged per RUN of consecutive lanes: the
    // run's first lane reserves the run's ranks with one atomic. On a shuffled scene every run has length 1 (same
    // number of atomics as before, a few lane-mask instructions more).
    const bool emit = fits && n_dup && !big;
    const int nb = emit ? (cx1 - cx0) * (cy1 - cy0) : 0;
    unsigned dup = (unsigned)(base + ex);
    int cx = cx0, cy = cy0;
    if (pairs) {
      // TWO-PASS BINNING (round 3): the items go, with plain stores and the coarse bin in the upper half of the mask
      // word, into this workgroup's stretch of the pair list; bin_scatter_kernel then ranks them per bin with LDS
      // atomics and reserves slab ranges with ONE device atomic per (scatter workgroup, bin) -- 0.5 M instead of 2.7 M
      // returning device atomics on the headline scene, which is what this kernel was bound by.
      unsigned pos = blockIdx.x * (unsigned)PAIRS_PER_BLOCK + ex_items;
#pragma unroll
      for (int k = 0; k < BIG_WALK; ++k) {
        if (k < nb) {
          const unsigned m = (unsigned)((k < 4 ? mask_lo >> (16 * k) : mask_hi >> (16 * (k - 4))) & 0xffffull);
          if (m) {
            pairs[pos++] = make_uint4((unsigned)g, depth_bits, dup, m | ((unsigned)(cy * CX + cx) << 16));
            dup += (unsigned)__popc(m);
          }
          if (++cx == cx1) { cx = cx0; ++cy; }
        }
      }
      if (threadIdx.x == 0) block_items[blockIdx.x] = fits ? total_items : 0u;
    } else {
    const unsigned long long le = (2ull << lane) - 1ull;   // lanes <= this one
    for (int k = 0; __ballot(k < nb) != 0ull; ++k) {
      unsigned m = 0;
      if (k < nb) m = (unsigned)((k < 4 ? mask_lo >> (16 * k) : mask_hi >> (16 * (k - 4))) & 0xffffull);
      const int cb = cy * CX + cx;
      const unsigned key = m ? (unsigned)cb : 0x80000000u | (unsigned)lane;   // idle lanes break the runs
      const unsigned prev = (unsigned)__shfl_up((int)key, 1);
      const unsigned long long heads = __ballot(lane == 0 || key != prev);
      const int h = 63 - __clzll(heads & le);                      // first lane of this lane's run
      const unsigned long long above = heads & ~le;
      const int next = above ? __ffsll((long long)above) - 1 : 64;  // first lane of the next run
      // the counter is 64 bits wide: items appended in the low word (the returned value is the run's first rank), the
      // TILE hits of those items in the high word -- plan_scan turns the per-bin hit totals into list-slot bases, so that
      // fine_bin needs no allocator (2 040 returning atomics on one word were a third of its time)
      const unsigned pc = m ? (unsigned)__popc(m) : 0u;
      unsigned run_hits = pc;                      // every lane its own run (a shuffled scene): no scan needed
      if (heads != ~0ull) {                        // wave-uniform
        const unsigned pincl = wave_incl_scan_u32(pc);
        run_hits = (unsigned)__shfl((int)pincl, next - 1) - (pincl - pc);   // meaningful in lane h
      }
      unsigned rank0 = 0;
      // (the 64-bit atomic costs preprocess ~5 us on the shuffled headline scene -- 14 + 18 bits packed into a 32-bit
      // one ~3 us, not worth a capacity-dependent format -- against 20 us of allocator queueing removed from fine_bin)
      if (m && h == lane)
        rank0 = (unsigned)atomicAdd(reinterpret_cast<unsigned long long*>(&coarse_count[(size_t)cb * CC_STRIDE]),
                                    (unsigned long long)(unsigned)(next - h) | ((unsigned long long)run_hits << 32));
      rank0 = (unsigned)__shfl((int)rank0, h);
      if (m) {
        const unsigned rank = rank0 + (unsigned)(lane - h);
        if (rank < coarse_capacity) slabs[(size_t)cb * coarse_capacity + rank] = make_uint4((unsigned)g, depth_bits, dup, m);
        else hdr[HDR_OVERFLOW] = 1ull;
        dup += (unsigned)__popc(m);
      }
      if (k < nb && ++cx == cx1) { cx = cx0; ++cy; }
    }
    }
  }
  for (unsigned long long bl = fits ? big_lanes : 0ull; bl; bl &= bl - 1) {  // cooperative emission (fits is block-uniform)
    const int L = __builtin_ctzll(bl);
    const WalkArgs a = broadcast_walk(r, br, thr, cx0, cx1, cy0, cy1, L);
    const unsigned g_L = (unsigned)__shfl((int)g, L), depth_L = __shfl(depth_bits, L);
    unsigned dup = __shfl((unsigned)(base + ex), L);
    const int ncb = (a.cx1 - a.cx0) * (a.cy1 - a.cy0);
    // ONE returning atomic instruction per splat (round 4). The walk takes up to 16 iterations of four coarse bins (a
    // mid-size splat has < 64 of them); the item of (iteration it, group q) is appended by lane 16 q + it, which keeps the
    // iteration's mask / bin / first duplicate index when its turn comes -- so all of the splat's <= 63 atomics are in
    // flight TOGETHER and the wave waits for one round trip per splat instead of one per iteration (the near-camera
    // regime -- 200 k splats of ~36 coarse bins -- spent most of this kernel's 2.4 ms in those waits, one rank at a time).
    const int q = lane >> 4, turn = lane & 15;
    const unsigned long long below_q = (1ull << (16 * q)) - 1ull;
    unsigned m_mine = 0u, dp_mine = 0u;
    int cb_mine = 0;
    for (int it = 0; it * 4 < ncb; ++it) {
      int cb;
      const unsigned long long bal = walk_ballot4(a, it, lane, f.W, f.H, bound, &cb, CX);
      if (turn == it) {
        m_mine = (unsigned)(bal >> (16 * q)) & 0xffffu;
        cb_mine = cb;
        dp_mine = dup + (unsigned)__popcll(bal & below_q);
      }
      dup += (unsigned)__popcll(bal);
    }
    if (m_mine) {
      const unsigned rank = (unsigned)atomicAdd(reinterpret_cast<unsigned long long*>(&coarse_count[(size_t)cb_mine * CC_STRIDE]),
                                                1ull | ((unsigned long long)(unsigned)__popc(m_mine) << 32));
      if (rank < coarse_capacity) slabs[(size_t)cb_mine * coarse_capacity + rank] = make_uint4(g_L, depth_L, dp_mine, m_mine);
      else hdr[HDR_OVERFLOW] = 1ull;
    }
  }
  // per-block statistics (summed by plan_scan; no contended atomics)
  block_excl_scan_u32<PRE_BLOCK>(vis, &total, s_red);
  if (threadIdx.x == 0) block_nvis[blockIdx.x] = total;
  block_excl_scan_u32<PRE_BLOCK>(dref, &total, s_red);
  if (threadIdx.x == 0) block_dref[blockIdx.x] = total;
}

// ------------------------------------------------------------------------------------------------
// K1b: the binning walk of the splats preprocess_kernel listed as huge (64 coarse bins and more), ONE WAVE PER SPLAT,
// persistent waves over the work list. Two passes over the splat's coarse bins, lane = coarse bin: count the hit
// tiles, reserve the duplicate indices (one atomic per splat), then emit one item per non-empty coarse bin.
// (Mid-size splats stay with the wave that owns them: sent here too, every splat pays the latency chain list entry ->
// record -> walk -> atomic -> stores on its own, and a pitched camera's 600 k mid-size splats took 1.2 ms instead of 0.45.)
__global__ void __launch_bounds__(256)
big_walk_kernel(KFrame kf, const uint4* __restrict__ big_list, const float4* __restrict__ rec,
                uint2* __restrict__ dup_out, uint32_t* __restrict__ coarse_count, uint4* __restrict__ slabs,
                unsigned coarse_capacity, unsigned long long dup_capacity, uint2* __restrict__ big_chunks,
                unsigned big_chunk_cap, unsigned long long* __restrict__ hdr, unsigned long long* __restrict__ dup_pool,
                unsigned npools) {
  // the count pass leaves every coarse bin's 16-bit tile mask in LDS for the emit pass (round 4: the 16 tile tests per bin
  // were done twice); splats of more than BIG_WALK_CACHE coarse bins (images beyond ~2 K) recompute the tail
  __shared__ uint16_t bw_masks[4][BIG_WALK_CACHE];
  uint16_t* my_masks = bw_masks[threadIdx.x >> 6];
  const unsigned n_big = (unsigned)hdr[HDR_BIG_COUNT];
  const int lane = threadIdx.x & 63;
  const unsigned nwaves = gridDim.x * (blockDim.x >> 6);
  const int W = kf.W, H = kf.H;
  const int CX = (((W + TILE_BIN - 1) / TILE_BIN) + COARSE - 1) / COARSE;
  const float bound = __uint_as_float((unsigned)hdr[HDR_SUBPIX_BOUND]);
  for (unsigned i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); i < n_big; i += nwaves) {
    const uint4 it = big_list[i];
    const unsigned g = it.x;
    const float4 r0 = rec[REC_F4 * (size_t)g], r1 = rec[REC_F4 * (size_t)g + 1], r2 = rec[REC_F4 * (size_t)g + 2];
    WalkArgs a;
    a.r.mx = r0.x; a.r.my = r0.y; a.r.qa = r0.z; a.r.qb = r0.w; a.r.qc = r1.x; a.r.op = r1.y; a.r.depth = r2.y;
    a.r.r = a.r.g = a.r.b = 0.f; a.r.ex = r2.z; a.r.ey = r2.w;
    a.br.x0 = (int)(it.y & 0xffffu); a.br.x1 = (int)(it.y >> 16);
    a.br.y0 = (int)(it.z & 0xffffu); a.br.y1 = (int)(it.z >> 16);
    a.thr = alpha_threshold_log2(a.r.op);
    a.cx0 = a.br.x0 / COARSE; a.cx1 = (a.br.x1 - 1) / COARSE + 1;
    a.cy0 = a.br.y0 / COARSE; a.cy1 = (a.br.y1 - 1) / COARSE + 1;
    const unsigned depth_bits = __float_as_uint(a.r.depth);
    const int nx = a.cx1 - a.cx0, ncb = nx * (a.cy1 - a.cy0);
    // pass 1: count
    unsigned total = 0;   // lane = coarse bin (16 tile tests per lane and iteration, index math amortised)
    for (int i0 = 0; i0 < ncb; i0 += 64) {
      const int j = i0 + lane;
      unsigned c = 0;
      if (j < ncb) {
        const unsigned m = coarse_hits(a.r, a.thr, a.br, a.cx0 + j % nx, a.cy0 + j / nx, W, H, bound);
        if (j < BIG_WALK_CACHE) my_masks[j] = (uint16_t)m;
        c = (unsigned)__popc(m);
      }
      total += wave_sum_u32(c);
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    // reserve the duplicate indices
    unsigned long long base = 0ull;
    bool ok = true;
    if (lane == 0 && total) base = dup_alloc(dup_pool, npools, i, total, dup_capacity, &ok);
    base = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(base >> 32)) << 32) |
           (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)base);
    const bool fits = __builtin_amdgcn_readfirstlane((int)ok) != 0;
    if (lane == 0) {
      dup_out[g] = make_uint2((unsigned)base, total);
      if (!fits) hdr[HDR_OVERFLOW] = 1ull;
    }
    if (!fits || total == 0) continue;
    if (total > BWD_BIG) {  // list this Gaussian's records in chunks for the backward's parallel reduction
      const unsigned nch = (total + BWD_CHUNK - 1) / BWD_CHUNK;
      unsigned long long cb0 = 0ull;
      if (lane == 0) cb0 = atomicAdd(&hdr[HDR_BIG_CHUNKS], (unsigned long long)nch);
      const unsigned c0 = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)cb0);
      if ((unsigned long long)c0 + nch <= big_chunk_cap) {
        for (unsigned c = lane; c < nch; c += 64) big_chunks[c0 + c] = make_uint2(g, c);
      } else if (lane == 0) {
        hdr[HDR_OVERFLOW] = 1ull;   // cannot happen while dup_capacity >= D (big_chunk_capacity's bound); kept for safety
      }
    }
    // pass 2: emit
    unsigned dup = (unsigned)base;
    for (int i0 = 0; i0 < ncb; i0 += 64) {
      const int j = i0 + lane;
      unsigned m = 0;
      int cb = 0;
      if (j < ncb) {
        const int cx = a.cx0 + j % nx, cy = a.cy0 + j / nx;
        m = j < BIG_WALK_CACHE ? (unsigned)my_masks[j] : coarse_hits(a.r, a.thr, a.br, cx, cy, W, H, bound);
        cb = cy * CX + cx;
      }
      const unsigned c = (unsigned)__popc(m);
      const unsigned incl = wave_incl_scan_u32(c);
      if (m) {
        const unsigned rank = (unsigned)atomicAdd(reinterpret_cast<unsigned long long*>(&coarse_count[(size_t)cb * CC_STRIDE]),
                                                  1ull | ((unsigned long long)c << 32));
        if (rank < coarse_capacity) slabs[(size_t)cb * coarse_capacity + rank] = make_uint4(g, depth_bits, dup + incl - c, m);
        else hdr[HDR_OVERFLOW] = 1ull;
      }
      dup += __shfl(incl, 63);
    }
  }
}

void launch_subpix_bound(const float* subpix, int W, int H, unsigned long long* hdr, hipStream_t stream) {
  const int64_t n = (int64_t)W * H * 2;
  const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((n / 4 + 255) / 256, 512));
  hipLaunchKernelGGL(subpix_bound_kernel, dim3(blocks), dim3(256), 0, stream, subpix, n, hdr);
}

int plan_preprocess(const SfgsFrame* frame, const SfgsGaussians* g, int32_t* radii, const KFrame& kf, const GeomView& gv,
                    const TilesView& tv, const BinsView& bv, int64_t dup_capacity, int64_t coarse_capacity, bool two_pass,
                    hipStream_t stream) {
  const int N = g->count, NB = (int)pre_blocks(N);
  if (frame->subpixel_offset) {
    // (round 6 tried ONE launch for the clear and the reduction -- per-workgroup partial maxima that every preprocess wave
    // reduces: the launch saved is worth less than what the 31 250 waves pay for it, 88 -> 92 us for the three kernels;
    // profiles/r6_plan_head_merge_ab_not_kept.txt)
    { ProfScope ps_(KID_SUBPIX, stream);
      launch_subpix_bound(frame->subpixel_offset, kf.W, kf.H, tv.hdr, stream); }
    SFGS_POST_LAUNCH("subpix_bound", stream, frame->debug);
  }
  if (NB > 0) {
    { ProfScope ps_(KID_PREPROCESS, stream);
#define SFGS_LAUNCH_PRE_(K, D, RAW, CM)                                                                                \
  hipLaunchKernelGGL((preprocess_kernel<K, D, RAW, CM>), dim3(NB), dim3(PRE_BLOCK), 0, stream, kf, N, g->means3D,      \
                     g->scales, g->rotations, (const void*)g->opacities, g->filter_3D, (int)g->raw_f64_mask,           \
                     g->colors_precomp, g->shs, g->shs_rest, g->sh_dirs ? g->sh_dirs : g->sh_centers,                 \
                     g->sh_centers ? 1 : 0, radii, gv.rec, gv.dup, tv.coarse_count,                                    \
                     bv.slabs,                                                                                         \
                     (unsigned)coarse_capacity, (unsigned long long)dup_capacity, tv.block_nvis, tv.block_dref,        \
                     gv.big_list, tv.hdr, tv.dup_pool, two_pass ? bv.pairs : nullptr, gv.block_items)
#define SFGS_LAUNCH_PRE(K, D)                                                                                          \
  do {                                                                                                                 \
    if constexpr ((K) > 0) {                                                                                           \
      if ((g->sh_dirs || g->sh_centers) && g->shs_channel_major) { if (g->filter_3D) SFGS_LAUNCH_PRE_(K, D, true, 1); else SFGS_LAUNCH_PRE_(K, D, false, 1); break; } \
      if (g->sh_dirs || g->sh_centers) { if (g->filter_3D) SFGS_LAUNCH_PRE_(K, D, true, 2); else SFGS_LAUNCH_PRE_(K, D, false, 2); break; } \
    }                                                                                                                  \
    if (g->filter_3D) SFGS_LAUNCH_PRE_(K, D, true, 0); else SFGS_LAUNCH_PRE_(K, D, false, 0);                          \
  } while (0)
      SFGS_DISPATCH_SH(g->shs ? frame->sh_coeffs : 0, frame->sh_degree, SFGS_LAUNCH_PRE);
#undef SFGS_LAUNCH_PRE
#undef SFGS_LAUNCH_PRE_
      // the big splats' walk: persistent waves over the work list (returns at once when the list is empty; not launched
      // at all when the caller asserts there are none -- it checks counters.num_huge_splats afterwards)
      if (!(frame->launch_hints & SFGS_HINT_NO_HUGE_SPLATS))
      hipLaunchKernelGGL(big_walk_kernel, dim3(BIG_WALK_BLOCKS), dim3(256), 0, stream, kf, gv.big_list, gv.rec, gv.dup,
                         tv.coarse_count, bv.slabs, (unsigned)coarse_capacity, (unsigned long long)dup_capacity,
                         bv.big_chunks, (unsigned)big_chunk_capacity(dup_capacity), tv.hdr, tv.dup_pool,
                         dup_pools_used(NB));
    }
    SFGS_POST_LAUNCH("preprocess", stream, frame->debug);
  }
  return SFGS_OK;
}

}  // namespace sfgs
