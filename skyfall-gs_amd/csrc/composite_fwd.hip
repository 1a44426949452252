// composite_fwd.hip -- last stage of the forward's render (map of the forward: raster_fwd.hip): tile_order (the
// longest-first tile order, on the caller's hint; also the backward's, by last contributor) and composite_fwd (one wave
// per 8x8 tile, front to back, records staged through LDS). The backward's counterpart is composite_bwd.hip.
//
// Compile with -ffp-contract=off: FMA only where the source spells fmaf (raster_math.h).
#include "sfgs_internal.h"

namespace sfgs {

// Variants built, measured and not kept (A/B files; the code is in the history, not in this source):
//   composite_fwd: records gathered in piece order (the backward's trick)   profiles/r4_fwd_gather3_ab_not_kept.txt
//   composite_fwd: exact ellipse-vs-pixel-row strip test                     profiles/r4_fwd_strip_exact_ab_not_kept.txt

// Longest-first tile order of the compositing kernels (SFGS_HINT_TILE_ORDER; round 6). A compositing wave owns one tile from
// its first to its last list entry, and a frame is only ~4 rounds of such waves deep: whatever is still running when the
// queue is empty runs alone. On a uniform frame that tail is one average tile; on a city seen from above -- lists of 200
// entries everywhere, 1 500 along the facades that are seen edge-on -- the wave timeline (tools/timeline.py) has composite_fwd
// drain for 70 of its 240 us, and list scheduling of the measured tile times longest first (within each XCD's share of the
// image, which keeps the chunked XCD mapping and its L2 sharing) predicts 187 us; composite_bwd 405 -> 370.
// One workgroup per XCD: a counting sort of the XCD's tiles by key (list length / last contributor) into 64 classes of 16
// entries, longest first; tiles without work last (a 4-wave workgroup of composite_bwd then holds four lists of one class
// and returns its LDS when all four are done -- in image order 28 % of that frame's tiles have nothing to blend and their
// workgroup-mates keep the LDS). Inside a class the order is whatever the LDS atomics make it: tiles are independent, any
// order composites the same bits. (A STABLE sort -- image order inside a class, in runs of 64 tiles -- was built and measured
// worse: city at 75 degrees 1.21 -> 1.10 ms instead of -> 1.04, composite_fwd 0.235 instead of 0.208 ms. And uniform frames lose
// with either -- headline +6 %, dense 8 M +12 % when forced on, almost all of it in composite_bwd: a class is a sparse subset of
// the image, the tiles in flight no longer gather the same records (FETCH_SIZE on the dense frame: composite_bwd 1.65 -> 2.27 GB
// per launch, 788 -> 1 161 us; composite_fwd 1.22 -> 2.17 GB at an unchanged 440 us) -- which is why
// the order is a HINT the caller only gives for frames whose longest list is several times their mean. Dealing the CHUNKS to the XCDs by work as well -- the XCDs still finish 4 - 8 % apart -- was built
// (tools/variants/chunk_deal_by_work_r6.patch) and bought the two kernels 1.4 / 2.4 % by rocprofv3, less than its own two extra
// passes cost: not kept. profiles/r6_tile_order_ab.txt, section 5.)
template <bool PAIRS>   // PAIRS: key = tile_range[t].y (uint2 array), else a plain uint32 array (tile_kmax)
__global__ void __launch_bounds__(1024)
tile_order_kernel(int TX8, int TY8, int SX, int SY, const void* __restrict__ keys_, uint32_t* __restrict__ order, unsigned P,
                  unsigned long long* __restrict__ hdr, unsigned bit) {
  __shared__ unsigned hist[65], base[65];
  const unsigned x = blockIdx.x;
  if (threadIdx.x < 65) hist[threadIdx.x] = 0u;
  __syncthreads();
  const unsigned SXc = (unsigned)(SX + CHUNK_BX - 1) / CHUNK_BX, SYc = (unsigned)(SY + CHUNK_BY - 1) / CHUNK_BY;
  const unsigned nch = SXc * SYc;
  constexpr unsigned PERCH = CHUNK_BX * CHUNK_BY * 4;   // tiles per chunk
  auto tile_of = [&](unsigned i, unsigned* cls) -> unsigned {   // slot i of this XCD in image (chunk) order -> tile, class
    const unsigned c = (i / PERCH) * 8u + x, within = i % PERCH;
    const unsigned st = within >> 2, sub = within & 3u;
    const unsigned tx = ((c % SXc) * CHUNK_BX + st % CHUNK_BX) * 2u + (sub & 1u);
    const unsigned ty = ((c / SXc) * CHUNK_BY + st / CHUNK_BX) * 2u + (sub >> 1);
    if (c >= nch || tx >= (unsigned)TX8 || ty >= (unsigned)TY8) { *cls = 64u; return 0xffffffffu; }
    const unsigned t = ty * (unsigned)TX8 + tx;
    const unsigned key = PAIRS ? static_cast<const uint2*>(keys_)[t].y : static_cast<const uint32_t*>(keys_)[t];
    *cls = key == 0u ? 63u : 62u - min(62u, (key - 1u) >> 4);   // class 0: more than 992 entries ... class 62: 1 .. 16; 63: none
    return t;
  };
  for (unsigned i = threadIdx.x; i < P; i += 1024) {
    unsigned cls;
    tile_of(i, &cls);
    atomicAdd(&hist[cls], 1u);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned run = 0;
    for (int k = 0; k < 65; ++k) { base[k] = run; run += hist[k]; }
  }
  __syncthreads();
  for (unsigned i = threadIdx.x; i < P; i += 1024) {
    unsigned cls;
    const unsigned t = tile_of(i, &cls);
    order[(size_t)x * P + atomicAdd(&base[cls], 1u)] = t;
  }
  if (x == 0 && threadIdx.x == 0) atomicOr(&hdr[HDR_TILE_ORDER], (unsigned long long)bit);
}

// ------------------------------------------------------------------------------------------------
// K5: compositing. Workgroup = 4 independent waves = a 2x2 block of 8x8 tiles; DPP row q = lane >> 4 of
// a wave owns the 4x4 quadrant q of its tile (x = 4 (q & 1) + (lane & 3), y = 4 (q >> 1) + ((lane >> 2) & 3)).
// Records of 64 list entries at a time are gathered
// (48 B each) into a wave-private LDS stage and consumed with uniform-address (broadcast) reads.
// No barriers: a wave only ever reads what it wrote itself.
// Each quadrant walks its own compact list of the batch's entries: those whose alpha >= 1/255 bounding box (mx +- ex,
// my +- ey) reaches the quadrant in x AND y. (Round 20; before, the rows owned 8x2 strips tested on y alone. Work model,
// tools/workmodel, headline: list steps per entry 0.728 -> 0.674 in TRAIN's 32-entry halves, 0.707 -> 0.650 in 64-entry
// batches, i.e. -7.4 / -8.2 %; measured -4.2 % (TRAIN, 0.212 -> 0.203 ms) and -5.5 % (render, 0.190 -> 0.180 ms), bit-identical
// outputs; 58 -> 60 and 54 -> 56 VGPRs, no scratch. profiles/r20_fwd_quadrant_lists_ab.txt)
// TRAIN (a backward will follow): every pixel also records WHICH entries it blended, one bit per entry, and the
// wave stores one 8-byte word per pixel and 64-entry batch (image blob, `hitmask`): the backward then walks each
// pixel's own blended entries instead of re-testing every (pixel, entry) pair of the list (raster_bwd.hip).
template <bool TRAIN>
__global__ void __launch_bounds__(64 * CWG_WAVES)
composite_fwd_kernel(KFrame kf, int TX8, int TY8, int SX, int SY, const uint2* __restrict__ tile_range,
                     const uint32_t* __restrict__ sorted_id, const float4* __restrict__ rec,
                     float* __restrict__ out_color, float* __restrict__ out_depth, float* __restrict__ out_alpha,
                     uint32_t* __restrict__ n_contrib, float* __restrict__ final_T, float* __restrict__ dacc_out,
                     uint2* __restrict__ hitmask, uint32_t* __restrict__ tile_kmax, uint16_t* __restrict__ tile_dead,
                     const unsigned long long* __restrict__ hdr, const uint32_t* __restrict__ order, unsigned order_P) {
  __shared__ float4 stage[CWG_WAVES][64 * 3];
  __shared__ __attribute__((aligned(8))) unsigned char rowlist[CWG_WAVES][4][64];
  // wave-uniform (readfirstlane / blockIdx): the tile, its list range and every loop bound below are scalars -> scalar
  // loads, SGPR loop counters and s_cbranch instead of exec-mask loops
  int tx, ty, lw;
  if (order) {   // (launch-uniform) longest list first within the XCD's share of the image: tile_order_kernel
    const unsigned ot = ordered_tile<CWG_WAVES>(order, order_P, lw);
    if (ot == 0xffffffffu) return;
    ty = (int)(ot / (unsigned)TX8); tx = (int)(ot - (unsigned)ty * (unsigned)TX8);
  } else {
    int sbx, sby, wave;
    if (!composite_wave_role(SX, SY, sbx, sby, wave, lw)) return;   // a surplus workgroup of the padded grid
    tx = sbx * 2 + (wave & 1); ty = sby * 2 + (wave >> 1);
  }
  const int lane = threadIdx.x & 63;
  if (tx >= TX8 || ty >= TY8 || ty < kf.band0 || ty >= kf.band1) return;
  const int W = kf.W, H = kf.H;
  // lane -> pixel: DPP row q = lane >> 4 owns the 4x4 QUADRANT q of the tile (left / right = q & 1, top / bottom = q >> 1),
  // its 16 lanes the quadrant's pixels row by row. slot = the pixel's position in image order inside the tile, 8 y + x:
  // where the backward (lane = 8 y + x) expects this pixel's hit-mask word.
  const int qx = 4 * ((lane >> 4) & 1), qy = 4 * (lane >> 5);
  const int slot = 8 * (qy + ((lane >> 2) & 3)) + qx + (lane & 3);
  const int px = tx * 8 + (slot & 7), py = ty * 8 + (slot >> 3);
  const bool inside = px < W && py < H;
  const size_t pix = (size_t)py * W + px;
  const int t = ty * TX8 + tx;
  const uint2 tr = tile_range[t];
  const unsigned s = tr.x, e = tr.x + tr.y;
  const float bound = __uint_as_float((unsigned)hdr[HDR_SUBPIX_BOUND]);
  float sx = (float)px, sy = (float)py;
  // (an all-zero offset tensor -- what the reference's render() passes without --ray_jitter -- is not even loaded: px + 0 = px)
  if (kf.subpix && bound != 0.f && inside) { sx += kf.subpix[pix * 2]; sy += kf.subpix[pix * 2 + 1]; }
  PixelFwd ps;
  pixel_fwd_init(ps, inside);
  float4* st = stage[lw];
  // Software pipeline over batches of 64 list entries: the (dependent) id -> record gathers of batch i+1
  // are issued before batch i is composited, so their latency hides behind ~1600 VALU instructions.
  float4 n0 = make_float4(0.f, 0.f, 0.f, 0.f), n1 = n0, n2 = n0;
  unsigned id_next = 0;
  if (s + lane < e) {
    const unsigned id = sorted_id[s + lane];
    n0 = rec[REC_F4 * (size_t)id]; n1 = rec[REC_F4 * (size_t)id + 1]; n2 = rec[REC_F4 * (size_t)id + 2];
  }
  if (s + 64 + lane < e) id_next = sorted_id[s + 64 + lane];
  for (unsigned b = s; b < e; b += 64) {
    if (__ballot(ps.T > 0.f) == 0ull) break;  // every pixel of the tile is saturated
    const unsigned cnt = min(64u, e - b);
    st[lane * 3] = n0; st[lane * 3 + 1] = n1; st[lane * 3 + 2] = n2;
    const float stage_mx = n0.x, stage_my = n0.y, stage_ex = n2.z, stage_ey = n2.w;
    if (b + 64 + lane < e) {  // prefetch: records of the next batch, ids of the one after
      n0 = rec[REC_F4 * (size_t)id_next]; n1 = rec[REC_F4 * (size_t)id_next + 1]; n2 = rec[REC_F4 * (size_t)id_next + 2];
    }
    if (b + 128 + lane < e) id_next = sorted_id[b + 128 + lane];
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const unsigned k0 = b - s;
    // Quadrant skipping. Only ~25 % of the (pixel, splat) pairs of a tile list hit (splats of a few pixels on an 8x8
    // tile), and a wave cannot skip per lane -- but it can per DPP row: lanes 16q..16q+15 own the 4x4 quadrant q, and an
    // entry whose alpha >= 1/255 region (bounding box mx +- ex, my +- ey: fill_extents, margins included) misses the
    // quadrant's pixels in x or in y cannot be accepted by any of them. Each quadrant therefore walks its own compact list
    // of the batch entries that can touch it; the four quadrants advance in lockstep and the wave leaves the batch when the
    // longest list is exhausted. Exact: the skipped pairs are pairs the per-pixel test would have rejected. The negated
    // comparisons keep an entry with a NaN or infinite extent (NaN opacity: fill_extents) in every list.
    // (Until round 20 the rows owned 8x2 strips tested on y alone -- x adds nothing to a strip as wide as the tile: 0.728
    // list steps per entry on the headline against 0.674 for quadrants, tools/workmodel; same four ballots per batch.
    // Eight single-row lists needed fewer steps than the strips but twice the list set-up: same time.)
    const float mx = stage_mx, my = stage_my, ex = stage_ex, ey = stage_ey;   // this lane's STAGED entry (entry index = lane)
    const float xlo = (float)(tx * 8) - bound, xhi = (float)(tx * 8 + 3) + bound;
    const float ylo = (float)(ty * 8) - bound, yhi = (float)(ty * 8 + 3) + bound;
    const bool live = (unsigned)lane < cnt;
    const bool in_l = live && !(mx + ex < xlo) && !(mx - ex > xhi);                 // columns 0..3
    const bool in_r = live && !(mx + ex < xlo + 4.f) && !(mx - ex > xhi + 4.f);     // columns 4..7
    const bool in_t = !(my + ey < ylo) && !(my - ey > yhi);                         // rows 0..3
    const bool in_b = !(my + ey < ylo + 4.f) && !(my - ey > yhi + 4.f);             // rows 4..7
    const unsigned long long b0 = __ballot(in_l && in_t);
    const unsigned long long b1 = __ballot(in_r && in_t);
    const unsigned long long b2 = __ballot(in_l && in_b);
    const unsigned long long b3 = __ballot(in_r && in_b);
    // per-quadrant compact entry lists (bytes) in LDS
    unsigned char* Lw = &rowlist[lw][0][0];
    const int row = lane >> 4;
    const unsigned char* Lr = Lw + row * 64;
    if constexpr (!TRAIN) {
      // entry `lane` goes to position rank(lane) of every row it touches
      auto rank = [&](unsigned long long m) {
        return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
      };
      if ((b0 >> lane) & 1ull) Lw[0 * 64 + rank(b0)] = (unsigned char)lane;
      if ((b1 >> lane) & 1ull) Lw[1 * 64 + rank(b1)] = (unsigned char)lane;
      if ((b2 >> lane) & 1ull) Lw[2 * 64 + rank(b2)] = (unsigned char)lane;
      if ((b3 >> lane) & 1ull) Lw[3 * 64 + rank(b3)] = (unsigned char)lane;
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      const int n0r = __popcll(b0), n1r = __popcll(b1), n2r = __popcll(b2), n3r = __popcll(b3);
      const int len = row == 0 ? n0r : row == 1 ? n1r : row == 2 ? n2r : n3r;
      const int maxlen = max(max(n0r, n1r), max(n2r, n3r));
      for (int i = 0; i < maxlen; i += 8) {   // 8 list positions per early-exit check
        const uint2 j8 = *reinterpret_cast<const uint2*>(Lr + i);   // eight byte indices at once (i % 8 == 0)
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          if (i + u < len) {
            const unsigned j = ((u < 4 ? j8.x : j8.y) >> (8 * (u & 3))) & 0xffu;
            const float4 r0 = st[j * 3], r1 = st[j * 3 + 1];
            const float2 r2 = *reinterpret_cast<const float2*>(&st[j * 3 + 2]);
            const SplatEval ev = eval_splat(r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, sx, sy);
            pixel_fwd_step(ps, ev, r2.y, r1.z, r1.w, r2.x, k0 + j);
          }
        }
        if (__ballot(ps.T > 0.f) == 0ull) break;
      }
    } else {
      // The batch is walked as two halves of 32 entries (row lists: positions 0.. for entries 0..31, positions 32..
      // for entries 32..63), so that a pixel's blended-entry bits of one half live in ONE 32-bit register and the
      // bit index is the entry index itself (v_lshl_or uses the low five bits of j).
      auto pos = [&](unsigned long long m) {
        const unsigned lo = __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u);
        const unsigned hi = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), 0u);
        return lane < 32 ? lo : 32u + hi;
      };
      if ((b0 >> lane) & 1ull) Lw[0 * 64 + pos(b0)] = (unsigned char)lane;
      if ((b1 >> lane) & 1ull) Lw[1 * 64 + pos(b1)] = (unsigned char)lane;
      if ((b2 >> lane) & 1ull) Lw[2 * 64 + pos(b2)] = (unsigned char)lane;
      if ((b3 >> lane) & 1ull) Lw[3 * 64 + pos(b3)] = (unsigned char)lane;
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      unsigned mlo = 0u, mhi = 0u;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int n0r = __popc((unsigned)(b0 >> (32 * half))), n1r = __popc((unsigned)(b1 >> (32 * half)));
        const int n2r = __popc((unsigned)(b2 >> (32 * half))), n3r = __popc((unsigned)(b3 >> (32 * half)));
        const int len = row == 0 ? n0r : row == 1 ? n1r : row == 2 ? n2r : n3r;
        const int maxlen = max(max(n0r, n1r), max(n2r, n3r));
        unsigned& m = half ? mhi : mlo;
        bool done = false;
        for (int i = 0; i < maxlen; i += 8) {
          const uint2 j8 = *reinterpret_cast<const uint2*>(Lr + 32 * half + i);
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            if (i + u < len) {
              const unsigned j = ((u < 4 ? j8.x : j8.y) >> (8 * (u & 3))) & 0xffu;
              const float4 r0 = st[j * 3], r1 = st[j * 3 + 1];
              const float2 r2 = *reinterpret_cast<const float2*>(&st[j * 3 + 2]);
              const SplatEval ev = eval_splat(r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, sx, sy);
              pixel_fwd_step_mask(ps, ev, r2.y, r1.z, r1.w, r2.x, j, m);
            }
          }
          if (__ballot(ps.T > 0.f) == 0ull) { done = true; break; }
        }
        if (done) break;
      }
      if (mlo | mhi) ps.last = k0 + (mhi ? 63u - (unsigned)__clz(mhi) : 31u - (unsigned)__clz(mlo)) + 1u;
      hitmask[(size_t)b + slot] = make_uint2(mlo, mhi);   // b is a multiple of 64: one 512-byte store per batch, word 8 y + x
    }
    __builtin_amdgcn_wave_barrier();
  }
  const float T = pixel_fwd_final_T(ps), C0 = ps.C0, C1 = ps.C1, C2 = ps.C2, D = ps.D;
  const unsigned last = ps.last;
  if constexpr (TRAIN) {  // the tile's last contributor: where the backward starts, and how much of the list is dead
    unsigned kmax = last;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) kmax = max(kmax, (unsigned)__shfl_xor((int)kmax, d));
    if (lane == 0) {
      tile_kmax[t] = kmax;
      // (summed by dupgrad_prefill_kernel. One device atomic per tile on a frame counter instead: 32 400 atomics on one
      // address serialise at ~9 ns each -- near-camera regime: 0.13 -> 0.42 ms)
      tile_dead[t] = (uint16_t)min(e - s - kmax, 65535u);
    }
  }
  if (inside) {
    const size_t P = (size_t)W * H;
    out_color[pix] = fmaf(T, kf.bg[0], C0);
    out_color[P + pix] = fmaf(T, kf.bg[1], C1);
    out_color[2 * P + pix] = fmaf(T, kf.bg[2], C2);
    const float a = 1.0f - T;
    out_alpha[pix] = a;
    out_depth[pix] = kf.depth_mode == SFGS_DEPTH_NORMALISED ? D / a : D;
    if constexpr (TRAIN) { n_contrib[pix] = last; final_T[pix] = T; dacc_out[pix] = D; }
  }
}

int composite_forward(const SfgsFrame* frame, const KFrame& kf, const GeomView& gv, const TilesView& tv, const BinsView& bv,
                      const ImageView* iv, float* out_color, float* out_depth, float* out_alpha, hipStream_t stream) {
  const int W = kf.W, H = kf.H, TX8 = tiles8_x(W), TY8 = tiles8_y(H);
  const int SX = (TX8 + 1) / 2, SY = (TY8 + 1) / 2;
  const unsigned cgrid = composite_grid(SX, SY, 4 / CWG_WAVES);
  // longest-first tile order (tile_order_kernel): asked for by the caller's hint, forced / forbidden by the "tile_order" option
  const unsigned OP = (unsigned)order_slots(W, H);
  const bool ordered = option(OPT_TILE_ORDER) == 1 || (option(OPT_TILE_ORDER) == 0 && (frame->launch_hints & SFGS_HINT_TILE_ORDER));
  const uint32_t* ord = ordered ? tv.tile_order : nullptr;
  { ProfScope ps_(KID_COMPOSITE_FWD, stream);
    if (ordered)
      hipLaunchKernelGGL(tile_order_kernel<true>, dim3(8), dim3(1024), 0, stream, TX8, TY8, SX, SY, (const void*)tv.tile_range,
                         tv.tile_order, OP, tv.hdr, 1u);
    if (iv) {
      hipLaunchKernelGGL(composite_fwd_kernel<true>, dim3(cgrid), dim3(64 * CWG_WAVES), 0, stream, kf, TX8, TY8, SX, SY,
                         tv.tile_range, bv.sorted_id, gv.rec, out_color, out_depth, out_alpha, iv->n_contrib, iv->final_T,
                         iv->dacc, iv->hitmask, iv->tile_kmax, iv->tile_dead, tv.hdr, ord, OP);
      if (ordered)   // the backward's order, by last contributor (known now)
        hipLaunchKernelGGL(tile_order_kernel<false>, dim3(8), dim3(1024), 0, stream, TX8, TY8, SX, SY, (const void*)iv->tile_kmax,
                           tv.tile_order + (size_t)8 * OP, OP, tv.hdr, 2u);
    } else {
      hipLaunchKernelGGL(composite_fwd_kernel<false>, dim3(cgrid), dim3(64 * CWG_WAVES), 0, stream, kf, TX8, TY8, SX, SY,
                         tv.tile_range, bv.sorted_id, gv.rec, out_color, out_depth, out_alpha, (uint32_t*)nullptr,
                         (float*)nullptr, (float*)nullptr, (uint2*)nullptr, (uint32_t*)nullptr, (uint16_t*)nullptr, tv.hdr,
                         ord, OP);
    } }
  SFGS_POST_LAUNCH("composite_fwd", stream, frame->debug);
  return SFGS_OK;
}

}  // namespace sfgs
